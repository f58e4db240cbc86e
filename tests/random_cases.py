"""Random meshes and states for the randomised GPU parity tests (a plain module, imported by the tests that need it).

Meshes: irregular triangles (jittered vertices, random diagonals), jittered convex quads, and mixed meshes of quads and split
quads in random patches (triangles padded with -1 in the 4-vertex connectivity).  States: every branch of the arithmetic --
dry and nearly-dry cells around tiny_h, thin films, supercritical and transcritical jumps, inflow through critical-outflow
edges -- drawn cell by cell, or region-blocked: runs of consecutive cells (which the tile cutter turns into whole tiles) that are
all dry, all around tiny_h, all thin film or all supercritical, next to runs of ordinary cells, so that consecutive tiles of
one workgroup differ in edge count, halo count and branch mix."""
import numpy as np

from rdycore_amd import cases as CS
from rdycore_amd import mesh as M

# the classes of cell random_case draws from (Case.cell_kind)
KIND_DRY, KIND_TINY, KIND_FILM, KIND_DEEP = 0, 1, 2, 3
KIND_NAMES = {KIND_DRY: "dry", KIND_TINY: "tiny_h", KIND_FILM: "film", KIND_DEEP: "deep"}


def _grid_vertices(rng, nx, ny, jitter):
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    x = ii.ravel().astype(float)
    y = jj.ravel().astype(float)
    inner = (ii.ravel() > 0) & (ii.ravel() < nx) & (jj.ravel() > 0) & (jj.ravel() < ny)
    x[inner] += rng.uniform(-jitter, jitter, inner.sum())
    y[inner] += rng.uniform(-jitter, jitter, inner.sum())
    z = 0.3 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.05 * rng.normal(size=x.size)
    return np.stack([x, y, z], axis=1)


def _tri_conn(rng, nx, ny):
    v = lambda i, j: j * (nx + 1) + i
    conn = []
    for j in range(ny):
        for i in range(nx):
            if rng.random() < 0.5:
                conn += [[v(i, j), v(i + 1, j), v(i + 1, j + 1)], [v(i, j), v(i + 1, j + 1), v(i, j + 1)]]
            else:
                conn += [[v(i, j), v(i + 1, j), v(i, j + 1)], [v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)]]
    return np.array(conn, dtype=np.int32)


def random_tri_mesh(rng, nx, ny, project_2d=False):
    xyz = _grid_vertices(rng, nx, ny, 0.3)
    conn = _tri_conn(rng, nx, ny)
    conn = conn[rng.permutation(conn.shape[0])]
    return M.build_mesh(xyz, conn, boundary_classifier=M.box_side_boundaries(0, nx, 0, ny), project_2d=project_2d)


def quads_are_convex(xyz, conn):
    """True where a 4-vertex cell (counter-clockwise) turns left at each of its corners; triangles (-1 pad) count as convex"""
    conn = np.asarray(conn)
    quad = conn[:, 3] >= 0
    q = conn[quad]
    p = xyz[q][:, :, :2]                                          # [n, 4, 2]
    a = np.roll(p, -1, axis=1) - p                                # edge k: corner k -> k+1
    b = np.roll(a, -1, axis=1)                                    # edge k+1
    cross = a[:, :, 0] * b[:, :, 1] - a[:, :, 1] * b[:, :, 0]
    ok = np.ones(conn.shape[0], dtype=bool)
    ok[quad] = (cross > 0).all(axis=1)
    return ok


def _quad_conn(nx, ny):
    v = lambda i, j: j * (nx + 1) + i
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    i, j = i.ravel(), j.ravel()
    return np.stack([v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)], axis=1).astype(np.int32)


def random_quad_mesh(rng, nx, ny, project_2d=False, permute=True):
    """nx x ny unit quads with every interior vertex moved by up to 0.2 in x and y (a corner angle then stays below 180
    degrees: every quad is convex, which is checked), cells in random order unless permute=False"""
    xyz = _grid_vertices(rng, nx, ny, 0.2)
    conn = _quad_conn(nx, ny)
    assert quads_are_convex(xyz, conn).all()
    if permute:
        conn = conn[rng.permutation(conn.shape[0])]
    return M.build_mesh(xyz, conn, boundary_classifier=M.box_side_boundaries(0, nx, 0, ny), project_2d=project_2d)


def random_mixed_conn(rng, nx, ny, patch=4):
    """connectivity of a mixed mesh: patches of patch x patch quads are kept whole or split (each quad along a random
    diagonal into two triangles, -1 in the fourth vertex as test_gpu_parity's mixed mesh pads them)"""
    q = _quad_conn(nx, ny)
    i = np.arange(nx * ny) % nx
    j = np.arange(nx * ny) // nx
    npx, npy = (nx + patch - 1) // patch, (ny + patch - 1) // patch
    split_patch = rng.random((npy, npx)) < 0.5
    split = split_patch[j // patch, i // patch]
    diag = rng.random(nx * ny) < 0.5
    conn = []
    for k in range(nx * ny):
        a, b, c, d = q[k]
        if not split[k]:
            conn.append([a, b, c, d])
        elif diag[k]:
            conn += [[a, b, c, -1], [a, c, d, -1]]
        else:
            conn += [[a, b, d, -1], [b, c, d, -1]]
    return np.array(conn, dtype=np.int32)


def random_mixed_mesh(rng, nx, ny, project_2d=False, permute=True, patch=4):
    xyz = _grid_vertices(rng, nx, ny, 0.2)
    conn = random_mixed_conn(rng, nx, ny, patch)
    assert quads_are_convex(xyz, conn).all()
    assert (conn[:, 3] < 0).any() and (conn[:, 3] >= 0).any()
    if permute:
        conn = conn[rng.permutation(conn.shape[0])]
    return M.build_mesh(xyz, conn, boundary_classifier=M.box_side_boundaries(0, nx, 0, ny), project_2d=project_2d)


def random_connectivity(rng, kind, nx, ny):
    """(xyz, conn) of a random mesh of `kind` ("tri", "quad", "mixed") in source order, for M.extract_local_mesh"""
    if kind == "tri":
        return _grid_vertices(rng, nx, ny, 0.3), _tri_conn(rng, nx, ny)
    xyz = _grid_vertices(rng, nx, ny, 0.2)
    conn = _quad_conn(nx, ny) if kind == "quad" else random_mixed_conn(rng, nx, ny)
    assert quads_are_convex(xyz, conn).all()
    return xyz, conn


def random_mesh(rng, kind, nx, ny, project_2d=False, permute=True):
    """a random mesh of `kind` ("tri", "quad", "mixed"): cells in random order (tiles of few cells, halos as large as the
    tile capacities allow) or, permute=False, in row-major order (full tiles)"""
    if kind == "tri":
        if permute:
            return random_tri_mesh(rng, nx, ny, project_2d=project_2d)
        xyz, conn = random_connectivity(rng, kind, nx, ny)
        return M.build_mesh(xyz, conn, boundary_classifier=M.box_side_boundaries(0, nx, 0, ny), project_2d=project_2d)
    if kind == "quad":
        return random_quad_mesh(rng, nx, ny, project_2d=project_2d, permute=permute)
    return random_mixed_mesh(rng, nx, ny, project_2d=project_2d, permute=permute)


def random_partition_mesh(rng, kind, nx, ny, project_2d=False):
    """one rank's local mesh of a random global mesh: the owned cells are a band across the middle of the domain with a
    hole in it, ghosts interleaved with them in the row-major source order (a DMPlex-like local numbering: the owned cells
    are not a prefix, F and u_out rows are scattered); tiles away from the band's edges and the hole have no ghost-adjacent
    cell and run in the INTERIOR phase"""
    xyz, conn = random_connectivity(rng, kind, nx, ny)
    nv = (conn >= 0).sum(axis=1)
    cx = np.where(conn >= 0, xyz[np.maximum(conn, 0), 0], 0.0).sum(axis=1) / nv
    cy = np.where(conn >= 0, xyz[np.maximum(conn, 0), 1], 0.0).sum(axis=1) / nv
    hole = (np.abs(cx - 0.5 * nx) < 0.08 * nx) & (np.abs(cy - 0.5 * ny) < 0.08 * ny)
    owned = (cy >= 0.2 * ny) & (cy < 0.8 * ny) & ~hole
    return M.extract_local_mesh(xyz, conn, owned, boundary_classifier=M.box_side_boundaries(0, nx, 0, ny),
                                ghosts="interleaved", project_2d=project_2d)


def _block_kinds(rng, nc, cfg, block):
    """one class per run of `block` consecutive cells: ordinary (-1: drawn cell by cell), dry, tiny_h, thin film or
    supercritical deep water"""
    nb = (nc + block - 1) // block
    choices = np.array([-1, -1, KIND_DRY, KIND_TINY, KIND_FILM, 4])
    if cfg.second_order:
        choices = np.array([-1, -1, KIND_DRY, 4])
    bk = rng.choice(choices, nb)
    bk[0] = -1                                      # the walk starts on an ordinary tile
    return np.repeat(bk, block)[:nc]


def random_case(rng, mesh, cfg, region_block=0):
    """a random state, sources, friction and boundary data on `mesh`.  region_block > 0: the classes of cell are dealt in
    runs of that many consecutive local cells (region-blocked); 0: cell by cell.  The class of every local cell is left on
    the case as `cell_kind` (KIND_*)."""
    nc = mesh.num_cells
    kind = rng.integers(0, 5, nc)
    if cfg.second_order:
        # linear extrapolation next to films of 1e-7..1e-2 m gives velocities of 1e6 m/s and |F| ~ 1e11 in the reference
        # too, which would make the relative L-inf bar meaningless: dry or deep cells only
        kind = np.where((kind == 1) | (kind == 2), 3, kind)
    if region_block > 0:
        bk = _block_kinds(rng, nc, cfg, region_block)
        kind = np.where(bk == 4, 3, np.where(bk >= 0, bk, kind))
    h = np.where(kind == 0, 0.0,                                        # dry
        np.where(kind == 1, cfg.tiny_h * rng.uniform(0.2, 3.0, nc),     # around the wet/dry threshold
        np.where(kind == 2, rng.uniform(1e-4, 1e-2, nc),                # thin films
                 rng.uniform(0.2, 3.0, nc))))                           # deep
    speed = np.where(rng.random(nc) < 0.3, rng.uniform(3.0, 12.0, nc), rng.uniform(0.0, 1.5, nc))   # some supercritical
    if region_block > 0:
        speed = np.where(bk == 4, rng.uniform(6.0, 12.0, nc), speed)    # supercritical blocks
    ang = rng.uniform(0, 2 * np.pi, nc)
    u = np.stack([h, h * speed * np.cos(ang), h * speed * np.sin(ang)], axis=1)
    ctypes, bvals = [], {}
    for i, b in enumerate(mesh.boundaries):
        t = [M.CONDITION_DIRICHLET, M.CONDITION_REFLECTING, M.CONDITION_CRITICAL_OUTFLOW, M.CONDITION_DIRICHLET][i % 4]
        ctypes.append(t)
        if t == M.CONDITION_DIRICHLET:
            hb = np.where(rng.random(b.num_edges) < 0.2, 0.0, rng.uniform(0.1, 2.0, b.num_edges))
            bvals[i] = np.stack([hb, hb * rng.normal(size=b.num_edges), hb * rng.normal(size=b.num_edges)], axis=1)
    no = mesh.num_owned_cells
    src = rng.normal(size=(no, 3)) * np.array([1e-4, 1e-3, 1e-3])
    case = CS.Case("fuzz", mesh, cfg, ctypes, u, rng.uniform(0.01, 0.06, no), src, bvals, float(rng.choice([1e-3, 1e-2, 0.1])))
    case.cell_kind = np.where(kind >= 3, KIND_DEEP, kind)
    return case
