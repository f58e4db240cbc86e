"""GPU parity: the HIP operator (through the C ABI) against the CPU oracle on the
same seeded inputs.  Tolerance: RHS L-inf <= 1e-10 relative to max(1, |F|_inf)
(BASELINE.json north_star); achieved values are ~1e-15.
"""
import numpy as np
import pytest

from rdycore_amd import mesh as M
from rdycore_amd import cases as CS
from rdycore_amd.operator import SOURCE_IMPLICIT_XQ2018, SOURCE_SEMI_IMPLICIT

from helpers import oracle_from_case, rel_linf

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def run_both(case, accumulate_from=None, check_diag=True):
    """Returns (F_gpu, F_oracle, op, orc) after one RHS evaluation."""
    torch = _torch()
    orc = oracle_from_case(case)
    op = CS.create_operator(case)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    no = case.mesh.num_owned_cells
    if accumulate_from is None:
        f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")  # must be overwritten, never read
        op.rhs_function(case.dt, u, f)
        f_ref = orc.apply(case.dt, case.u_local)
    else:
        f = torch.tensor(accumulate_from, dtype=torch.float64, device="cuda")
        op.reset_diagnostics()
        op.apply(case.dt, u, f)
        f_ref = orc.apply(case.dt, case.u_local, accumulate_from.copy())
    torch.cuda.synchronize()
    return f.cpu().numpy(), f_ref, op, orc


def check_all(case, f_gpu, f_ref, op, orc, near_tie_ok=False):
    err = rel_linf(f_gpu, f_ref)
    assert np.isfinite(f_ref).all()
    assert err <= TOL, f"{case.name}: RHS L-inf {err:.3e}"
    pv = op.primitive_variables.cpu().numpy()
    assert rel_linf(pv, orc.primitive_variables) <= TOL
    # Courant diagnostics (value to rounding, ids exactly)
    op.update_diagnostics()
    d = op.get_diagnostics()
    cmax, ce, cc = orc.diagnostics()
    # first order: the same arithmetic up to FMA contraction.  Second order: the gradients are formed as M^-1 (sum w d dq) on
    # the chip instead of sum (M^-1 w d) dq with host-made coefficients -- equal by linearity, different by cond(M) x rounding,
    # which unlimited extrapolation on jittered meshes passes on to the wave speeds; the bar there is the RHS's 1e-10
    ctol = 1e-10 if case.config.second_order else 1e-12
    assert abs(d.max_courant_num - cmax) <= ctol * max(1.0, cmax)
    if case.mesh.num_owned_cells == case.mesh.num_cells and (d.global_edge_id, d.global_cell_id) != (ce, cc):
        # Another edge than the oracle's: only legitimate if the reference's own Courant numbers of the two edges agree to
        # rounding (mirror-image edges of a symmetric state: which of them comes out on top hangs on the last bits of sin()
        # at the two centroids, and the device's last bits -- FMA contraction, its own square roots -- are not the oracle's).
        # Edges that tie EXACTLY in the reference (uniform states) must give the reference's edge: near_tie_ok is off there.
        assert near_tie_ok and not case.config.second_order, ((d.global_edge_id, d.global_cell_id), (ce, cc))
        from helpers import interior_courant_numbers
        m = case.mesh
        c = interior_courant_numbers(case)
        pos = np.nonzero(m.edge_global_ids[m.edge_internal_ids] == d.global_edge_id)[0]
        assert pos.size == 1 and abs(c[pos[0]] - cmax) <= 1e-13 * cmax, ((d.global_edge_id, d.global_cell_id), (ce, cc))
        e = int(m.edge_internal_ids[pos[0]])
        l, r = int(m.edge_cell_ids[2 * e]), int(m.edge_cell_ids[2 * e + 1])
        assert d.global_cell_id == int(m.cell_global_ids[l if m.cell_areas[l] < m.cell_areas[r] else r])
    # boundary fluxes and their dt-weighted accumulation
    for b, bnd in enumerate(case.mesh.boundaries):
        bf = op.boundary_fluxes(b)
        ref = orc.boundary_fluxes[b]
        both_nan = np.isnan(bf) & np.isnan(ref)   # dry-dry edges are NaN in the reference too
        assert np.array_equal(np.isnan(bf), np.isnan(ref))
        assert rel_linf(np.where(both_nan, 0.0, bf), np.where(both_nan, 0.0, ref)) <= TOL
        ba = op.boundary_fluxes(b, accumulated=True)
        ra = orc.boundary_fluxes_accum[b]
        assert np.array_equal(np.isnan(ba), np.isnan(ra))
        assert rel_linf(np.nan_to_num(ba), np.nan_to_num(ra)) <= TOL
    return err


def tri_mms_case(nx, ny, source_method, order="rowmajor", dry=True):
    K = 2 * np.pi / (0.8 * nx)
    mesh = M.structured_tri_mesh(nx, ny, 1.0, zfunc=CS.mms_bathymetry(K=K), order=order, tile=4)
    return CS.friction_slope_case(mesh, nx, ny, dt=1e-2, source_method=source_method, dry_disc=dry, K=K)


@pytest.mark.parametrize("source_method", [SOURCE_SEMI_IMPLICIT, SOURCE_IMPLICIT_XQ2018])
@pytest.mark.parametrize("order", ["rowmajor", "tiled"])
def test_tri_all_bcs_sources(source_method, order):
    case = tri_mms_case(37, 23, source_method, order)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
    op.destroy()


def test_dam_break_tri():
    mesh = M.structured_tri_mesh(40, 20)
    case = CS.dam_break_case(mesh, 40.0)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)


def test_uniform_state_ties_pick_first_edge():
    # lake at rest on a flat bed: every edge has the same Courant number; the
    # reference reports the first edge in loop order.
    mesh = M.structured_tri_mesh(9, 7)
    case = CS.dam_break_case(mesh, 1e9, perturb=0.0)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)


@pytest.mark.parametrize("source_method", [SOURCE_SEMI_IMPLICIT, SOURCE_IMPLICIT_XQ2018])
def test_quad_mesh(source_method):
    K = 2 * np.pi / 20
    mesh = M.structured_quad_mesh(17, 11, 1.0, 1.5, zfunc=CS.mms_bathymetry(K=K))
    case = CS.friction_slope_case(mesh, 17.0, 16.5, dt=5e-3, source_method=source_method, K=K)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
    assert op.layout_info()["slots_per_cell"] == 4


def test_mixed_tri_quad_mesh():
    # left half quads, right half triangles: 4-slot layout with empty slots
    nx, ny = 10, 6
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    xyz = np.zeros(((nx + 1) * (ny + 1), 3))
    xyz[:, 0] = ii.ravel()
    xyz[:, 1] = jj.ravel()
    xyz[:, 2] = 0.05 * np.sin(xyz[:, 0]) + 0.02 * xyz[:, 1]
    v = lambda i, j: j * (nx + 1) + i
    conn = []
    for j in range(ny):
        for i in range(nx):
            if i < nx // 2:
                conn.append([v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)])
            else:
                conn.append([v(i, j), v(i + 1, j), v(i + 1, j + 1), -1])
                conn.append([v(i, j), v(i + 1, j + 1), v(i, j + 1), -1])
    mesh = M.build_mesh(xyz, np.array(conn, dtype=np.int32), boundary_classifier=M.box_side_boundaries(0, nx, 0, ny))
    case = CS.friction_slope_case(mesh, nx, ny, dt=1e-2, K=2 * np.pi / 9, dry_disc=True)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)


def test_accumulate_semantics_match_apply_operator():
    # ApplyOperator adds into f_global and the friction term sees the incoming
    # content through the flux-divergence copy (src/operator.c:663)
    case = tri_mms_case(21, 13, SOURCE_SEMI_IMPLICIT)
    rng = np.random.default_rng(7)
    f0 = rng.normal(size=(case.mesh.num_owned_cells, 3)) * 0.1
    f, fr, op, orc = run_both(case, accumulate_from=f0)
    assert rel_linf(f, fr) <= TOL


@pytest.mark.parametrize("ghosts", ["tail", "interleaved"])
def test_partition_with_ghost_cells(ghosts):
    # one rank's local mesh (owned + ghost cells, ghosts pre-filled): only owned
    # cells are written, shared edges use the ghost state
    nxg, ny = 24, 10
    K = 2 * np.pi / 15
    xyz, conn, cqi, _ = M.structured_tri_connectivity(nxg, ny)
    xyz[:, 2] = CS.mms_bathymetry(K=K)(xyz[:, 0], xyz[:, 1])
    owned = (cqi >= 8) & (cqi < 16)
    mesh = M.extract_local_mesh(xyz, conn, owned, boundary_classifier=M.box_side_boundaries(0, nxg, 0, ny), ghosts=ghosts)
    assert mesh.num_cells > mesh.num_owned_cells
    case = CS.friction_slope_case(mesh, nxg, ny, dt=1e-2, K=K, dry_disc=True)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
    info = op.layout_info()
    assert info["owned_is_prefix"] == (1 if ghosts == "tail" else 0)
    assert info["num_halo_cells"] > 0

    # phased apply (interior cells, then halo cells) gives the same answer
    torch = _torch()
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f2 = torch.zeros((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.reset_diagnostics()
    op.reset_boundary_fluxes_accum()
    op.apply_phase(1, True, case.dt, u, f2)
    op.apply_phase(2, True, case.dt, u, f2)
    torch.cuda.synchronize()
    assert np.array_equal(f2.cpu().numpy(), f)
    op.update_diagnostics()
    assert abs(op.get_diagnostics().max_courant_num - orc.diagnostics()[0]) <= 1e-12
    # the local half of DMGlobalToLocal (rdyhip_copy_owned_rows): the owned rows of a global vector land in their local
    # rows (a contiguous prefix or scattered), ghost rows are left alone
    ug = torch.tensor(np.random.default_rng(3).random((mesh.num_owned_cells, 3)), dtype=torch.float64, device="cuda")
    ul = torch.full((mesh.num_cells, 3), -7.0, dtype=torch.float64, device="cuda")
    op.copy_owned_rows(ug, ul)
    torch.cuda.synchronize()
    want = np.full((mesh.num_cells, 3), -7.0)
    want[mesh.cell_owned_to_local] = ug.cpu().numpy()
    assert np.array_equal(ul.cpu().numpy(), want)


def test_dry_bed_and_nan_free_rhs():
    # everything dry except a strip: dry-dry edges produce NaN fluxes that must
    # never reach F
    mesh = M.structured_tri_mesh(16, 8)
    case = CS.dam_break_case(mesh, 16.0)
    case.u_local[mesh.cell_centroids[:, 0] > 6.0] = 0.0
    f, fr, op, orc = run_both(case)
    assert np.isfinite(f).all()
    check_all(case, f, fr, op, orc)


def test_setters_regional_and_components():
    torch = _torch()
    mesh = M.structured_tri_mesh(8, 5)
    case = CS.dam_break_case(mesh, 8.0)
    op = CS.create_operator(case)
    orc = oracle_from_case(case)
    ids = np.arange(3, 40, 4, dtype=np.int32)
    vals = np.linspace(0.1, 0.9, ids.size)
    op.set_regional_external_source(ids, 1, vals)
    orc.external_sources[ids, 1] = vals
    op.set_regional_mannings_n(ids, 0.03 + vals * 0.01)
    orc.mannings[ids] = 0.03 + vals * 0.01
    assert np.array_equal(op.external_sources.cpu().numpy(), orc.external_sources)
    assert np.array_equal(op.mannings_n.cpu().numpy(), orc.mannings)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f = torch.zeros((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.enable_flux_divergence(True)
    op.rhs_function(case.dt, u, f)
    fr = orc.apply(case.dt, case.u_local)
    torch.cuda.synchronize()
    assert rel_linf(f.cpu().numpy(), fr) <= TOL
    assert rel_linf(op.flux_divergence.cpu().numpy(), orc.flux_divergence) <= TOL


def test_stream_ordered_setters():
    """rdyhip_set_*_on / rdyhip_refresh_field (no device synchronisation, pinned staging, the operator's copy stream): the fields
    end up as the synchronising setters leave them; a launch enqueued BEFORE the call still sees the old values, one enqueued
    after it the new ones; the host array is free again when the call returns; more refreshes in flight than staging slots"""
    torch = _torch()
    K = 2 * np.pi / 31
    mesh = M.structured_tri_mesh(40, 30, 1.0, zfunc=CS.mms_bathymetry(K=K))
    case = CS.friction_slope_case(mesh, 40.0, 30.0, dt=1e-2, K=K)
    op, ref = CS.create_operator(case), CS.create_operator(case)
    no = mesh.num_owned_cells
    rng = np.random.default_rng(11)
    ids = np.sort(rng.choice(no, size=no // 3, replace=False)).astype(np.int32)
    s = torch.cuda.Stream()
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f_old, f_new, f_ref = (torch.empty((no, 3), dtype=torch.float64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        op.rhs_function(case.dt, u, f_old)                       # enqueued before the refresh: the old inputs
        for rep in range(7):                                     # 7 x 4 staged arrays through a ring of 4 slots
            scratch = rng.random(no)
            op.set_domain_external_source(0, scratch, ordered=True)
            scratch[:] = np.nan                                  # free again: the call has copied it
            vals = rng.random(ids.size)
            op.set_regional_external_source(ids, 1, vals, ordered=True)
            man = 0.02 + 0.01 * rng.random(no)
            op.set_domain_mannings_n(man, ordered=True)
            b = mesh.boundary_by_name("left") if any(bd.name == "left" for bd in mesh.boundaries) else 0
            bv = np.abs(rng.normal(size=(mesh.boundaries[b].num_edges, 3))) + 0.5
            op.set_boundary_values(b, bv[:, :2], ordered=True)
            op.set_boundary_values(b, bv[:, 2], comp_offset=2, ordered=True)
        op.rhs_function(case.dt, u, f_new)
    # the same final inputs through the synchronising setters on a second operator
    src0 = rng.random(no)
    ref.set_domain_external_source(0, src0)
    op.set_domain_external_source(0, src0, ordered=False)        # the legacy call orders itself against everything
    ref.set_regional_external_source(ids, 1, vals)
    ref.set_domain_mannings_n(man)
    ref.set_boundary_values(b, bv)
    s.synchronize()
    for name in ("external_sources", "mannings_n"):
        assert torch.equal(getattr(op, name), getattr(ref, name)), name
    ref.rhs_function(case.dt, u, f_ref)
    with torch.cuda.stream(s):
        op.rhs_function(case.dt, u, f_new)
    torch.cuda.synchronize()
    assert torch.equal(f_new, f_ref)
    orc = oracle_from_case(case)
    assert rel_linf(f_old.cpu().numpy(), orc.apply(case.dt, case.u_local)) <= TOL       # untouched by the refreshes behind it
    # whole-field refresh from a host array and from a device tensor
    ext = rng.random((no, 3))
    op.refresh_field(1, ext)
    op.refresh_field(2, torch.tensor(man[::-1].copy(), device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(op.external_sources.cpu().numpy(), ext) and np.array_equal(op.mannings_n.cpu().numpy(), man[::-1])
    from rdycore_amd.operator import RDyHipError
    with pytest.raises(RDyHipError):
        op.refresh_field(1, ext[:-1])                            # size is checked against the field
    with pytest.raises(RDyHipError):
        op.refresh_field(0, ext)                                 # outputs cannot be written
    with pytest.raises(RDyHipError):
        op.set_regional_external_source(np.array([no], dtype=np.int32), 0, np.zeros(1), ordered=True)
    op.destroy(); ref.destroy()


def test_stream_ordered_setters_of_large_arrays():
    """the staged path in chunks (arrays above 8 MB go host -> pinned -> device chunk by chunk, the uploads beside the host
    copies): 2.6 M cells = 2.6 chunks of values, a regional list with ids behind the values in the same slot, a field refresh of
    7.8 chunks; several in flight, the host arrays scribbled over right after each call"""
    torch = _torch()
    mesh = M.structured_tri_mesh(1300, 1000, 1.0, order="tiled")
    case = CS.friction_slope_case(mesh, 1300.0, 1000.0, dt=1e-3)
    op = CS.create_operator(case)
    no = mesh.num_owned_cells
    rng = np.random.default_rng(5)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for rep in range(3):
            rain = rng.random(no)
            keep_rain = rain.copy()
            op.set_domain_external_source(0, rain, ordered=True)
            rain[:] = np.nan
            ids = np.sort(rng.choice(no, size=no - 12345, replace=False)).astype(np.int32)
            vals = rng.random(ids.size)
            keep_vals = vals.copy()
            op.set_regional_external_source(ids, 2, vals, ordered=True)
            vals[:] = np.nan
            man = 0.02 + 0.01 * rng.random(no)
            keep_man = man.copy()
            op.set_domain_mannings_n(man, ordered=True)
            man[:] = np.nan
    s.synchronize()
    ext = op.external_sources.cpu().numpy()
    assert np.array_equal(ext[:, 0], keep_rain) and np.array_equal(ext[ids, 2], keep_vals) and np.array_equal(op.mannings_n.cpu().numpy(), keep_man)
    whole = rng.random((no, 3))
    keep = whole.copy()
    with torch.cuda.stream(s):
        op.refresh_field(1, whole)
        whole[:] = np.nan
    s.synchronize()
    assert np.array_equal(op.external_sources.cpu().numpy(), keep)
    op.destroy()


def test_cached_f_stores_option_changes_nothing_but_the_cache_policy():
    """RDYHIP_CONFIG_CACHED_F_STORES (for hosts whose TSEULER reads F straight back): same bits"""
    torch = _torch()
    import copy
    K = 2 * np.pi / 31
    mesh = M.structured_tri_mesh(40, 30, 1.0, zfunc=CS.mms_bathymetry(K=K))
    case = CS.friction_slope_case(mesh, 40.0, 30.0, dt=1e-2, K=K)
    case2 = copy.copy(case)
    case2.config = copy.copy(case.config)
    case2.config.cached_f_stores = True
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    out = []
    for c in (case, case2):
        op = CS.create_operator(c)
        f = torch.empty((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
        op.rhs_function(c.dt, u, f)
        torch.cuda.synchronize()
        out.append(f)
        op.destroy()
    assert torch.equal(out[0], out[1])


def test_uout_store_policy_changes_nothing_but_the_cache_policy():
    """The Euler-step kernels store u_out with the default cache policy when the state fits the Infinity Cache and with the
    non-temporal hint when it does not (rdyhip_create decides by size; RDYHIP_UOUT_CACHED forces): the same bits either way,
    F requested or not, on a part with ghost cells.  (The HR instantiations of both policies are held against the oracle by the
    trajectory tests: levee, bowl, C5 -- small states, plain stores -- and the 10 M / 45 M-cell cases -- hinted stores.)"""
    import os
    torch = _torch()
    K = 2 * np.pi / 31
    mesh = M.strip_partition_tri_mesh(40, 30, 1, 3, 1.0, zfunc=CS.mms_bathymetry(K=K), order="tiled", tile=8)   # a part with ghost cells
    case = CS.friction_slope_case(mesh, 120.0, 30.0, dt=1e-2, K=K)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    out = []
    for policy in ("0", "1"):
        os.environ["RDYHIP_UOUT_CACHED"] = policy
        try:
            op = CS.create_operator(case)
        finally:
            os.environ.pop("RDYHIP_UOUT_CACHED")
        a, b = u.clone(), u.clone()          # (the ghost rows of both arrays hold a valid state: a step writes owned rows only)
        f = torch.empty((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
        op.euler_step(case.dt, a, b, f)
        op.euler_step(case.dt, b, a)
        torch.cuda.synchronize()
        out.append((a, b, f))
        op.destroy()
    for x, y in zip(*out):
        assert torch.equal(torch.nan_to_num(x, nan=1e300), torch.nan_to_num(y, nan=1e300))
    own = torch.as_tensor(mesh.cell_owned_to_local.astype(np.int64), device="cuda")
    assert not torch.equal(torch.nan_to_num(out[0][0][own], nan=1e300), u[own])      # the steps did move the state


def test_error_behaviour():
    from rdycore_amd.operator import Operator, RDyFlowConfig, RDyHipError
    torch = _torch()
    mesh = M.structured_tri_mesh(4, 3)
    with pytest.raises(RDyHipError):
        Operator.create(RDyFlowConfig(riemann=2), mesh)          # "Unsupported Riemann solver"
    with pytest.raises(RDyHipError):
        Operator.create(RDyFlowConfig(source_method=2), mesh)    # ARK-IMEX is not a PETSc-path source
    op = Operator.create(RDyFlowConfig(), mesh)
    with pytest.raises(RDyHipError):
        op.set_boundary_values(0, np.zeros((mesh.boundaries[0].num_edges + 1, 3)))
    with pytest.raises(RDyHipError):
        op.set_boundary_values(99, np.zeros((1, 3)))
    u = torch.zeros((mesh.num_cells, 2), dtype=torch.float64, device="cuda")
    f = torch.zeros((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(RDyHipError):
        op.apply(0.1, u, f)
    op.destroy()


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_random_cell_numbering(kind):
    # a numbering with no locality: every tile's neighbours are almost all outside the tile
    # (the tiles are then cut small enough for the kernel's fixed halo capacity: csrc/host_layout.h, layout_cut_tiles)
    rng = np.random.default_rng(3)
    K = 2 * np.pi / 31
    if kind == "tri":
        xyz, conn, _, _ = M.structured_tri_connectivity(40, 30)
    else:
        base = M.structured_quad_mesh(36, 25)
        xyz, conn = base.xyz.copy(), base.cell_conn.copy()
    xyz[:, 2] = CS.mms_bathymetry(K=K)(xyz[:, 0], xyz[:, 1])
    conn = conn[rng.permutation(conn.shape[0])]
    lx, ly = xyz[:, 0].max(), xyz[:, 1].max()
    mesh = M.build_mesh(xyz, conn, boundary_classifier=M.box_side_boundaries(0, lx, 0, ly))
    case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2, K=K)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
    info = op.layout_info()
    if info["tiled_kernel"]:      # tiles of ~30 cells: three edge records and three halo cells per cell, cut at the halo capacity
        assert info["num_edge_records"] > 2.9 * mesh.num_cells and 90 <= info["max_tile_halo_cells"] <= 112
        assert info["num_tiles"] > mesh.num_cells // 48


# ---------------------------------------------------------------------------
# hydrostatic reconstruction (src/swe/swe_petsc.c:1000-1263)
# ---------------------------------------------------------------------------
def hr_case(kind, source_method):
    from rdycore_amd.operator import WELL_BALANCING_HR
    K = 2 * np.pi / 19
    z = lambda x, y: 0.6 * np.sin(K * x) * np.sin(K * y) + 0.02 * x      # bumps tall enough to leave islands
    if kind == "tri":
        mesh = M.structured_tri_mesh(33, 21, 1.0, zfunc=z, order="tiled", tile=4, project_2d=True)
        lx, ly = 33, 21
    else:
        mesh = M.structured_quad_mesh(21, 13, 1.0, 1.5, zfunc=z, project_2d=True)
        lx, ly = 21, 19.5
    case = CS.friction_slope_case(mesh, lx, ly, dt=1e-2, source_method=source_method, K=K, dry_disc=True)
    # shallow water over the bumps: some cells dry, some reconstructed depths clipped to zero
    eta = 0.45
    h = np.maximum(0.0, eta - mesh.cell_zc) * (1 + 0.2 * np.sin(0.7 * mesh.cell_centroids[:, 0]))
    uu = case.u_local[:, 1] / np.maximum(case.u_local[:, 0], 1e-12)
    vv = case.u_local[:, 2] / np.maximum(case.u_local[:, 0], 1e-12)
    case.u_local = np.stack([h, h * uu, h * vv], axis=1)
    case.config.well_balancing = WELL_BALANCING_HR
    return case


@pytest.mark.parametrize("kind", ["tri", "quad"])
@pytest.mark.parametrize("source_method", [SOURCE_SEMI_IMPLICIT, SOURCE_IMPLICIT_XQ2018])
def test_hydrostatic_reconstruction_parity(kind, source_method, rdyhip_kernel):
    if rdyhip_kernel == "cell":
        from rdycore_amd.operator import RDyHipError
        with pytest.raises(RDyHipError):
            CS.create_operator(hr_case(kind, source_method))     # HR lives in the tiled kernel only
        return
    case = hr_case(kind, source_method)
    assert (case.u_local[:, 0] == 0).any() and (case.u_local[:, 0] > 0.1).any()
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
    # accumulate semantics too
    f0 = np.random.default_rng(11).normal(size=fr.shape) * 0.01
    f2, fr2, op2, orc2 = run_both(case, accumulate_from=f0)
    assert rel_linf(f2, fr2) <= TOL


def test_hydrostatic_reconstruction_with_zero_length_edges(rdyhip_kernel):
    """edges of length zero (collapsed sides of a degenerate mesh: coefficient -0.0 on the left cell, +0.0 on the right)
    among interior and boundary edges: the HR kernel picks a slot's side from the coefficient's SIGN BIT and keeps the
    right-hand flux copy of boundary edges defined, so such a slot adds exactly 0 -- as in the oracle -- whatever the LDS
    held before (two evaluations with a NaN-producing state in between)"""
    if rdyhip_kernel == "cell":
        pytest.skip("HR lives in the tiled kernel")
    torch = _torch()
    case = hr_case("tri", SOURCE_SEMI_IMPLICIT)
    m = case.mesh
    rng = np.random.default_rng(4)
    zero = np.concatenate([rng.choice(m.edge_internal_ids, 40, replace=False), rng.choice(m.edge_boundary_ids, 12, replace=False)])
    m.edge_lengths = m.edge_lengths.copy()
    m.edge_lengths[zero] = 0.0
    orc = oracle_from_case(case)
    fr = orc.apply(case.dt, case.u_local)
    op = CS.create_operator(case)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f = torch.empty((m.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    bad = u.clone()
    bad[::7, 0] = float("nan")                      # leaves NaN fluxes behind in LDS
    op.rhs_function(case.dt, bad, f)
    op.rhs_function(case.dt, u, f)
    torch.cuda.synchronize()
    assert np.isfinite(fr).all() and rel_linf(f.cpu().numpy(), fr) <= TOL


def test_hydrostatic_reconstruction_lake_at_rest(rdyhip_kernel):
    if rdyhip_kernel == "cell":
        pytest.skip("HR lives in the tiled kernel")
    torch = _torch()
    from rdycore_amd.operator import WELL_BALANCING_HR
    K = 2 * np.pi / 9
    mesh = M.structured_tri_mesh(40, 30, 1.0, zfunc=lambda x, y: 0.3 * np.sin(K * x) * np.cos(K * y), order="tiled", tile=4, project_2d=True)
    case = CS.dam_break_case(mesh, 1e9, perturb=0.0)
    case.u_local[:, 0] = 2.0 - mesh.cell_zc
    case.config.well_balancing = WELL_BALANCING_HR
    op = CS.create_operator(case)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    f = torch.empty((mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.rhs_function(case.dt, u, f)
    assert float(f.abs().max()) < 1e-12


@pytest.mark.parametrize("z0", [500.0, 3000.0])
def test_hydrostatic_reconstruction_at_mountain_elevations(z0, rdyhip_kernel):
    """the HR edge phase takes ONE square root per edge -- the side with the higher bed keeps (h + z) - z and its
    staged sqrt(h) stands in for the root of that value (src/swe/swe_petsc.c:1046-1071 takes the root of the reconstructed depth):
    a relative difference of at most ulp(h + z) / (4 h), which grows with the bed's elevation and shrinks with the depth.
    Films of 1e-4 .. 1e-2 m (and deeper water, and dry cells) over a rough bed at 500 m and at 3000 m: still inside 1e-10."""
    if rdyhip_kernel == "cell":
        pytest.skip("HR lives in the tiled kernel")
    from rdycore_amd.operator import WELL_BALANCING_HR
    rng = np.random.default_rng(int(z0))
    K = 2 * np.pi / 17
    mesh = M.structured_tri_mesh(48, 36, 1.0, zfunc=lambda x, y: z0 + 0.8 * np.sin(K * x) * np.cos(K * y) + 0.03 * y, order="tiled", tile=4, project_2d=True)
    case = CS.dam_break_case(mesh, 1e9, perturb=0.0)
    nc = mesh.num_cells
    kind = rng.integers(0, 4, nc)
    h = np.where(kind == 0, 0.0, np.where(kind == 1, 10.0 ** rng.uniform(-4, -2, nc), np.where(kind == 2, rng.uniform(0.05, 0.5, nc), rng.uniform(0.5, 2.5, nc))))
    case.u_local[:, 0] = h
    case.u_local[:, 1] = h * rng.normal(size=nc) * 0.3
    case.u_local[:, 2] = h * rng.normal(size=nc) * 0.3
    case.config.well_balancing = WELL_BALANCING_HR
    f, fr, op, orc = run_both(case)
    err = check_all(case, f, fr, op, orc)
    # (measured: ~1e-13 at 500 m and at 3000 m -- the films that see the largest relative difference carry the smallest fluxes)
    assert err <= 1e-11
    op.destroy()


def test_hydrostatic_reconstruction_with_negative_depths(rdyhip_kernel):
    """a cell with a slightly negative depth (a drying overshoot) on the higher-bed side of an edge.  The
    reference clamps the reconstructed depth to 0 and takes sqrt(0) = 0 (src/swe/swe_petsc.c:1051-1053): a finite flux.  The staged
    square root of a negative depth is NaN; the one-root shortcut must not pass it on."""
    if rdyhip_kernel == "cell":
        pytest.skip("HR lives in the tiled kernel")
    case = hr_case("tri", SOURCE_SEMI_IMPLICIT)
    m = case.mesh
    rng = np.random.default_rng(12)
    # (not on the domain boundary: boundary edges are not reconstructed, src/operator_fluxes_petsc.c:57-58, and pow(h, 0.5) of a
    # negative depth is NaN there in the reference as well)
    on_boundary = np.zeros(m.num_cells, dtype=bool)
    on_boundary[m.edge_cell_ids[2 * m.edge_boundary_ids]] = True
    wet = np.nonzero((case.u_local[:, 0] > 0.05) & ~on_boundary)[0]
    neg = rng.choice(wet, 60, replace=False)
    case.u_local[neg, 0] = -10.0 ** rng.uniform(-9, -5, neg.size)
    case.u_local[neg, 1:] = 0.0
    # ... some of them certainly higher than a wet neighbour
    cl, cr = m.edge_cell_ids[2 * m.edge_internal_ids], m.edge_cell_ids[2 * m.edge_internal_ids + 1]
    isneg = np.zeros(m.num_cells, dtype=bool)
    isneg[neg] = True
    high_neg = (isneg[cl] & ~isneg[cr] & (m.cell_zc[cl] > m.cell_zc[cr]) & (case.u_local[cr, 0] > 0.05)) | \
               (isneg[cr] & ~isneg[cl] & (m.cell_zc[cr] > m.cell_zc[cl]) & (case.u_local[cl, 0] > 0.05))
    assert high_neg.sum() > 10
    f, fr, op, orc = run_both(case)
    assert np.isfinite(fr).all() and np.isfinite(f).all()
    assert rel_linf(f, fr) <= TOL
    op.destroy()


def test_unsupported_well_balancing_is_rejected():
    from rdycore_amd.operator import Operator, RDyFlowConfig, RDyHipError
    _torch()
    with pytest.raises(RDyHipError):
        Operator.create(RDyFlowConfig(well_balancing=1), M.structured_tri_mesh(4, 3))   # BS2002: CEED only (src/operator.c:388)


# ---------------------------------------------------------------------------
# edge cases: empty and ragged inputs
# ---------------------------------------------------------------------------
def test_rank_with_no_owned_cells():
    # a rank may own nothing (more ranks than cells): every call is a no-op
    torch = _torch()
    from rdycore_amd.operator import Operator, RDyFlowConfig
    xyz, conn, _, _ = M.structured_tri_connectivity(3, 2)
    mesh = M.build_mesh(xyz, conn, is_owned=np.zeros(conn.shape[0], dtype=np.int32), boundary_classifier=M.box_side_boundaries(0, 3, 0, 2))
    assert mesh.num_owned_cells == 0 and mesh.num_cells == 12
    op = Operator.create(RDyFlowConfig(), mesh)
    u = torch.ones((mesh.num_cells, 3), dtype=torch.float64, device="cuda")
    f = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    op.rhs_function(0.1, u, f)
    op.apply(0.1, u, f)
    op.update_diagnostics()
    d = op.get_diagnostics()
    assert (d.max_courant_num, d.global_edge_id, d.global_cell_id) == (0.0, -1, -1)   # ResetOperatorDiagnostics values
    assert op.primitive_variables.shape[0] == 0
    op.destroy()


def test_single_cell_and_empty_boundaries():
    # one triangle: three boundary edges spread over boundaries of 2, 1 and 0 edges
    xyz = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.1], [0.0, 1.0, 0.3]])
    conn = np.array([[0, 1, 2]], dtype=np.int32)

    def cls(mesh):
        be = mesh.edge_boundary_ids
        return [M.RDyBoundary(1, "two", be[:2].astype(np.int32)), M.RDyBoundary(2, "one", be[2:].astype(np.int32)),
                M.RDyBoundary(3, "none", np.zeros(0, dtype=np.int32))]

    mesh = M.build_mesh(xyz, conn, boundary_classifier=cls)
    from rdycore_amd.operator import RDyFlowConfig
    case = CS.Case("one_cell", mesh, RDyFlowConfig(source_method=SOURCE_IMPLICIT_XQ2018),
                   [M.CONDITION_REFLECTING, M.CONDITION_DIRICHLET, M.CONDITION_CRITICAL_OUTFLOW],
                   np.array([[1.3, 0.4, -0.2]]), np.array([0.03]), np.array([[1e-4, 0.0, 2e-4]]),
                   {1: np.array([[0.9, 0.1, 0.05]])}, 0.01)
    f, fr, op, orc = run_both(case)
    check_all(case, f, fr, op, orc)
    assert op.boundary_fluxes(2).shape == (0, 3)


def test_nan_state_propagates_like_the_reference():
    # a NaN depth is "not dry" for every guard (!(h < tiny_h)): it poisons exactly the cells the reference poisons
    mesh = M.structured_tri_mesh(12, 8)
    case = CS.dam_break_case(mesh, 12.0)
    case.u_local[37, 0] = np.nan
    f, fr, op, orc = run_both(case)
    assert np.array_equal(np.isnan(f), np.isnan(fr))
    ok = ~np.isnan(fr)
    assert np.isnan(fr).any() and rel_linf(f[ok], fr[ok]) <= TOL


def test_repeated_applies_and_persistent_diagnostics():
    # diagnostics persist across applies until reset (src/operator.c:772-784); boundary accumulations add up
    torch = _torch()
    case = tri_mms_case(19, 11, SOURCE_SEMI_IMPLICIT)
    op = CS.create_operator(case)
    orc = oracle_from_case(case)
    u1 = case.u_local.copy()
    u2 = case.u_local.copy()
    u2[:, 1:] *= 3.0                                  # faster flow: larger Courant number
    f = torch.zeros((case.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
    op.reset_diagnostics()
    for uu in (u2, u1):                               # the larger value comes first and must survive the second apply
        f.zero_()
        op.apply(case.dt, torch.tensor(uu, dtype=torch.float64, device="cuda"), f)
        orc.apply(case.dt, uu)
    op.update_diagnostics()
    d = op.get_diagnostics()
    cmax, ce, cc = orc.diagnostics()
    assert abs(d.max_courant_num - cmax) <= 1e-12 and (d.global_edge_id, d.global_cell_id) == (ce, cc)
    for b in range(len(case.mesh.boundaries)):
        assert rel_linf(np.nan_to_num(op.boundary_fluxes(b, accumulated=True)), np.nan_to_num(orc.boundary_fluxes_accum[b])) <= TOL
