"""One oracle comparison per instantiation of the RHS kernels, and the persistent tile walk on many-tile meshes.

ROWS names every template-argument tuple the library builds (test_kernel_matrix_cpu.py holds the table against the
instantiations of the built library) and how a host reaches it: mesh kind (slots per cell), source method, well balancing,
second order and limiter, RDYHIP_CONFIG_CACHED_F_STORES, RDYHIP_UOUT_CACHED and the call.  Every row runs on a random mesh
and state of random_cases.py -- owned cells as a prefix of the local numbering, or scattered between interleaved ghosts (the
o2l path), in one call or in the INTERIOR / HALO phases -- and is held against the CPU oracle: F (on a poisoned buffer, or
accumulated onto a random f0), the flux divergence, pv, the Courant value and ids, the boundary fluxes and their
accumulation; an Euler step by u_out = u + dt F_oracle.  The bar is the project's, rel L-inf <= 1e-10 against
max(1, |ref|), on the whole state and on each class of cell of the generator (dry, around tiny_h, thin film, deep) with its
own normalisation, so that an error confined to (nearly) dry cells cannot hide under the large |F| of supercritical ones.

WALK_CASES: meshes of many tiles (below 64 -- no XCD chunks --, exactly 64, above 64 with num_tiles % 8 == 1 / 7, a multiple
of 8) under a covering set of the walk's knobs (RDYHIP_PGRID 8 / 24, so that every workgroup walks many tiles; XCD chunks on
and off; balanced rounds; 64- and 256-cell tiles; the shrunken INTERIOR grid), first order, HR and second order in RHS and
Euler-step form: against the oracle, and bit for bit against the default-knob run of the same case."""
import dataclasses
import functools

import numpy as np
import pytest

from rdycore_amd import cases as CS
from rdycore_amd.operator import PHASE_ALL, PHASE_HALO, PHASE_INTERIOR, RDyFlowConfig

from helpers import oracle_from_case, rel_linf
from random_cases import KIND_NAMES, random_case, random_mesh, random_partition_mesh
from test_gpu_parity import check_all

pytestmark = pytest.mark.gpu
TOL = 1e-10
T, F = True, False
MM, NO, VL = 0, 1, 2          # limiters


@dataclasses.dataclass(frozen=True)
class Row:
    kernel: tuple             # ("tiled", S, SRC, OVERWRITE, HR, EULER, FNT) | ("muscl", S, SRC, OVERWRITE, LIM, EULER) | ("cell", S, SRC)
    mesh: str                 # tri (S = 3) | quad | mixed (S = 4)
    source_method: int
    well_balancing: int
    second_order: bool
    limiter: int
    cached_f_stores: bool
    uout_cached: object       # RDYHIP_UOUT_CACHED before create: 0 / 1, None = unset
    call: str                 # rhs (rdyhip_rhs_function) | apply (rdyhip_apply, accumulate) | euler (rdyhip_euler_step)
    layout: str               # prefix: owned cells first, no ghosts | o2l: ghosts interleaved with the owned cells
    phased: bool              # INTERIOR then HALO call instead of one

    @property
    def id(self):
        return "-".join(str(int(a) if isinstance(a, bool) else a) for a in self.kernel) + f"-{self.mesh}-{self.call}-{self.layout}" + \
            ("-phased" if self.phased else "")


#   kernel template arguments              mesh     src wb  2nd lim cachedF uout call      layout     phased
ROWS = [
    Row(("tiled", 3, 0, T, F, F, T), "tri",    0, 0, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 3, 0, T, F, F, F), "tri",    0, 0, F, MM, T, None, "rhs",     "o2l",     T),
    Row(("tiled", 3, 0, T, T, F, T), "tri",    0, 2, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 3, 0, T, T, F, F), "tri",    0, 2, F, MM, T, None, "rhs",     "o2l",     F),
    Row(("tiled", 3, 0, F, F, F, T), "tri",    0, 0, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 3, 0, F, F, F, F), "tri",    0, 0, F, MM, T, None, "apply",   "o2l",     T),
    Row(("tiled", 3, 0, F, T, F, T), "tri",    0, 2, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 3, 0, F, T, F, F), "tri",    0, 2, F, MM, T, None, "apply",   "o2l",     F),
    Row(("tiled", 3, 1, T, F, F, T), "tri",    1, 0, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 3, 1, T, F, F, F), "tri",    1, 0, F, MM, T, None, "rhs",     "o2l",     T),
    Row(("tiled", 3, 1, T, T, F, T), "tri",    1, 2, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 3, 1, T, T, F, F), "tri",    1, 2, F, MM, T, None, "rhs",     "o2l",     F),
    Row(("tiled", 3, 1, F, F, F, T), "tri",    1, 0, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 3, 1, F, F, F, F), "tri",    1, 0, F, MM, T, None, "apply",   "o2l",     T),
    Row(("tiled", 3, 1, F, T, F, T), "tri",    1, 2, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 3, 1, F, T, F, F), "tri",    1, 2, F, MM, T, None, "apply",   "o2l",     F),
    Row(("tiled", 4, 0, T, F, F, T), "mixed",  0, 0, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 4, 0, T, F, F, F), "mixed",  0, 0, F, MM, T, None, "rhs",     "o2l",     T),
    Row(("tiled", 4, 0, T, T, F, T), "quad",   0, 2, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 4, 0, T, T, F, F), "quad",   0, 2, F, MM, T, None, "rhs",     "o2l",     F),
    Row(("tiled", 4, 0, F, F, F, T), "quad",   0, 0, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 4, 0, F, F, F, F), "quad",   0, 0, F, MM, T, None, "apply",   "o2l",     T),
    Row(("tiled", 4, 0, F, T, F, T), "mixed",  0, 2, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 4, 0, F, T, F, F), "mixed",  0, 2, F, MM, T, None, "apply",   "o2l",     F),
    Row(("tiled", 4, 1, T, F, F, T), "quad",   1, 0, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 4, 1, T, F, F, F), "quad",   1, 0, F, MM, T, None, "rhs",     "o2l",     T),
    Row(("tiled", 4, 1, T, T, F, T), "mixed",  1, 2, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("tiled", 4, 1, T, T, F, F), "mixed",  1, 2, F, MM, T, None, "rhs",     "o2l",     F),
    Row(("tiled", 4, 1, F, F, F, T), "mixed",  1, 0, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 4, 1, F, F, F, F), "mixed",  1, 0, F, MM, T, None, "apply",   "o2l",     T),
    Row(("tiled", 4, 1, F, T, F, T), "quad",   1, 2, F, MM, F, None, "apply",   "prefix",  F),
    Row(("tiled", 4, 1, F, T, F, F), "quad",   1, 2, F, MM, T, None, "apply",   "o2l",     F),
    Row(("tiled", 3, 0, T, F, T, T), "tri",    0, 0, F, MM, F, 0, "euler",   "prefix",  F),
    Row(("tiled", 3, 0, T, F, T, F), "tri",    0, 0, F, MM, F, 1, "euler",   "prefix",  F),
    Row(("tiled", 3, 0, T, T, T, T), "tri",    0, 2, F, MM, F, 0, "euler",   "o2l",     T),
    Row(("tiled", 3, 0, T, T, T, F), "tri",    0, 2, F, MM, F, 1, "euler",   "o2l",     F),
    Row(("tiled", 3, 1, T, F, T, T), "tri",    1, 0, F, MM, F, 0, "euler",   "o2l",     T),
    Row(("tiled", 3, 1, T, F, T, F), "tri",    1, 0, F, MM, F, 1, "euler",   "o2l",     F),
    Row(("tiled", 3, 1, T, T, T, T), "tri",    1, 2, F, MM, F, 0, "euler",   "prefix",  F),
    Row(("tiled", 3, 1, T, T, T, F), "tri",    1, 2, F, MM, F, 1, "euler",   "prefix",  F),
    Row(("tiled", 4, 0, T, F, T, T), "quad",   0, 0, F, MM, F, 0, "euler",   "prefix",  F),
    Row(("tiled", 4, 0, T, F, T, F), "quad",   0, 0, F, MM, F, 1, "euler",   "prefix",  F),
    Row(("tiled", 4, 0, T, T, T, T), "mixed",  0, 2, F, MM, F, 0, "euler",   "o2l",     T),
    Row(("tiled", 4, 0, T, T, T, F), "mixed",  0, 2, F, MM, F, 1, "euler",   "o2l",     F),
    Row(("tiled", 4, 1, T, F, T, T), "mixed",  1, 0, F, MM, F, 0, "euler",   "o2l",     T),
    Row(("tiled", 4, 1, T, F, T, F), "mixed",  1, 0, F, MM, F, 1, "euler",   "o2l",     F),
    Row(("tiled", 4, 1, T, T, T, T), "quad",   1, 2, F, MM, F, 0, "euler",   "prefix",  F),
    Row(("tiled", 4, 1, T, T, T, F), "quad",   1, 2, F, MM, F, 1, "euler",   "prefix",  F),
    Row(("muscl", 3, 0, T, 0, F), "tri",    0, 0, T, MM, F, None, "rhs",     "o2l",     T),
    Row(("muscl", 3, 0, F, 0, F), "tri",    0, 0, T, MM, F, None, "apply",   "prefix",  F),
    Row(("muscl", 3, 0, T, 0, T), "tri",    0, 0, T, MM, F, None, "euler",   "prefix",  F),
    Row(("muscl", 3, 0, T, 1, F), "tri",    0, 0, T, NO, F, None, "rhs",     "o2l",     F),
    Row(("muscl", 3, 0, F, 1, F), "tri",    0, 0, T, NO, F, None, "apply",   "prefix",  F),
    Row(("muscl", 3, 0, T, 1, T), "tri",    0, 0, T, NO, F, None, "euler",   "prefix",  F),
    Row(("muscl", 3, 0, T, 2, F), "tri",    0, 0, T, VL, F, None, "rhs",     "o2l",     T),
    Row(("muscl", 3, 0, F, 2, F), "tri",    0, 0, T, VL, F, None, "apply",   "prefix",  F),
    Row(("muscl", 3, 0, T, 2, T), "tri",    0, 0, T, VL, F, None, "euler",   "prefix",  F),
    Row(("muscl", 3, 1, T, 0, F), "tri",    1, 0, T, MM, F, None, "rhs",     "o2l",     F),
    Row(("muscl", 3, 1, F, 0, F), "tri",    1, 0, T, MM, F, None, "apply",   "prefix",  F),
    Row(("muscl", 3, 1, T, 0, T), "tri",    1, 0, T, MM, F, None, "euler",   "prefix",  F),
    Row(("muscl", 3, 1, T, 1, F), "tri",    1, 0, T, NO, F, None, "rhs",     "o2l",     T),
    Row(("muscl", 3, 1, F, 1, F), "tri",    1, 0, T, NO, F, None, "apply",   "prefix",  F),
    Row(("muscl", 3, 1, T, 1, T), "tri",    1, 0, T, NO, F, None, "euler",   "prefix",  F),
    Row(("muscl", 3, 1, T, 2, F), "tri",    1, 0, T, VL, F, None, "rhs",     "o2l",     F),
    Row(("muscl", 3, 1, F, 2, F), "tri",    1, 0, T, VL, F, None, "apply",   "prefix",  F),
    Row(("muscl", 3, 1, T, 2, T), "tri",    1, 0, T, VL, F, None, "euler",   "prefix",  F),
    Row(("muscl", 4, 0, T, 0, F), "quad",   0, 0, T, MM, F, None, "rhs",     "o2l",     T),
    Row(("muscl", 4, 0, F, 0, F), "quad",   0, 0, T, MM, F, None, "apply",   "prefix",  F),
    Row(("muscl", 4, 0, T, 0, T), "quad",   0, 0, T, MM, F, None, "euler",   "prefix",  F),
    Row(("muscl", 4, 0, T, 1, F), "mixed",  0, 0, T, NO, F, None, "rhs",     "o2l",     F),
    Row(("muscl", 4, 0, F, 1, F), "mixed",  0, 0, T, NO, F, None, "apply",   "prefix",  F),
    Row(("muscl", 4, 0, T, 1, T), "mixed",  0, 0, T, NO, F, None, "euler",   "prefix",  F),
    Row(("muscl", 4, 0, T, 2, F), "quad",   0, 0, T, VL, F, None, "rhs",     "o2l",     T),
    Row(("muscl", 4, 0, F, 2, F), "quad",   0, 0, T, VL, F, None, "apply",   "prefix",  F),
    Row(("muscl", 4, 0, T, 2, T), "quad",   0, 0, T, VL, F, None, "euler",   "prefix",  F),
    Row(("muscl", 4, 1, T, 0, F), "mixed",  1, 0, T, MM, F, None, "rhs",     "o2l",     F),
    Row(("muscl", 4, 1, F, 0, F), "mixed",  1, 0, T, MM, F, None, "apply",   "prefix",  F),
    Row(("muscl", 4, 1, T, 0, T), "mixed",  1, 0, T, MM, F, None, "euler",   "prefix",  F),
    Row(("muscl", 4, 1, T, 1, F), "quad",   1, 0, T, NO, F, None, "rhs",     "o2l",     T),
    Row(("muscl", 4, 1, F, 1, F), "quad",   1, 0, T, NO, F, None, "apply",   "prefix",  F),
    Row(("muscl", 4, 1, T, 1, T), "quad",   1, 0, T, NO, F, None, "euler",   "prefix",  F),
    Row(("muscl", 4, 1, T, 2, F), "mixed",  1, 0, T, VL, F, None, "rhs",     "o2l",     F),
    Row(("muscl", 4, 1, F, 2, F), "mixed",  1, 0, T, VL, F, None, "apply",   "prefix",  F),
    Row(("muscl", 4, 1, T, 2, T), "mixed",  1, 0, T, VL, F, None, "euler",   "prefix",  F),
    Row(("cell", 3, 0), "tri",    0, 0, F, MM, F, None, "rhs",     "prefix",  F),
    Row(("cell", 3, 1), "tri",    1, 0, F, MM, F, None, "euler",   "o2l",     T),
    Row(("cell", 4, 0), "mixed",  0, 0, F, MM, F, None, "apply",   "o2l",     F),
    Row(("cell", 4, 1), "mixed",  1, 0, F, MM, F, None, "euler",   "prefix",  F),
]


def row_kernel(row):
    """the instantiation rdyhip_create / launch_rhs (rdyhip_api.hip) pick for a row: the selection restated"""
    S = 3 if row.mesh == "tri" else 4
    euler = row.call == "euler"
    ovw = row.call != "apply"
    if row.kernel[0] == "cell":
        return ("cell", S, row.source_method)
    if row.second_order:
        return ("muscl", S, row.source_method, ovw, row.limiter, euler)
    fnt = not bool(row.uout_cached) if euler else not row.cached_f_stores
    return ("tiled", S, row.source_method, ovw, row.well_balancing == 2, euler, fnt)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# ---- meshes: built once per module ------------------------------------------------------------------------------------------
_MATRIX_SIZE = {("tri", "prefix"): (36, 30), ("quad", "prefix"): (50, 44), ("mixed", "prefix"): (44, 36),
                ("tri", "o2l"): (60, 40), ("quad", "o2l"): (70, 56), ("mixed", "o2l"): (60, 44)}


@functools.lru_cache(maxsize=None)
def matrix_mesh(kind, layout, project_2d):
    """a few thousand cells: a random numbering (tiles of a few dozen cells, large halos; quads row-major: full tiles), or
    one rank's part with interleaved ghosts"""
    rng = np.random.default_rng({"tri": 11, "quad": 12, "mixed": 13}[kind] + (100 if layout == "o2l" else 0))
    nx, ny = _MATRIX_SIZE[(kind, layout)]
    if layout == "o2l":
        return random_partition_mesh(rng, kind, nx, ny, project_2d=project_2d)
    return random_mesh(rng, kind, nx, ny, project_2d=project_2d, permute=kind != "quad")


# ---- one evaluation on the device, the same on the oracle -------------------------------------------------------------------
def ghost_gradients(rng, case):
    """second order on a part with ghost cells: the ghost rows of the gradient field are the exchange's
    (CommunicateCellGradients) -- any values do, as long as device and oracle see the same"""
    mesh = case.mesh
    ghost = np.nonzero(mesh.cell_is_owned == 0)[0]
    if not case.config.second_order or ghost.size == 0:
        return None
    return ghost, rng.normal(size=(ghost.size, 6)) * np.array([0.1, 0.1, 0.3, 0.3, 0.3, 0.3])


def run_device(case, call, phased, f0=None, with_f=True, ggrad=None):
    """one rdyhip_rhs_function / rdyhip_apply / rdyhip_euler_step on a new operator (flux divergence kept);
    returns (op, F or None, u_out or None) on the host"""
    torch = _torch()
    mesh = case.mesh
    no = mesh.num_owned_cells
    op = CS.create_operator(case)
    op.enable_flux_divergence(True)
    u = torch.tensor(case.u_local, dtype=torch.float64, device="cuda")
    ready = case.config.second_order and (ggrad is not None or phased)
    if ready:
        if phased:
            op.compute_gradients(u, PHASE_INTERIOR)
            op.compute_gradients(u, PHASE_HALO)
        else:
            op.compute_gradients(u)
        if ggrad is not None:
            op.gradients[torch.as_tensor(ggrad[0], device="cuda")] = torch.as_tensor(ggrad[1], device="cuda")
    phases = (PHASE_INTERIOR, PHASE_HALO) if phased else (PHASE_ALL,)
    out = None
    if call == "euler":
        out = torch.full_like(u, -7.0)                                   # ghost rows must keep it
        f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda") if with_f else None
        for k, ph in enumerate(phases):
            op.euler_step(case.dt, u, out, f, phase=ph, reset_diagnostics=k == 0, gradients_ready=ready)
    else:
        overwrite = call == "rhs"
        if overwrite:
            f = torch.full((no, 3), 777.0, dtype=torch.float64, device="cuda")   # must be overwritten, never read
        else:
            f = torch.tensor(f0, dtype=torch.float64, device="cuda")
        if phased or ready:
            for k, ph in enumerate(phases):
                op.apply_phase(ph, overwrite, case.dt, u, f, reset_diagnostics=k == 0, gradients_ready=ready)
        elif overwrite:
            op.rhs_function(case.dt, u, f)
        else:
            op.reset_diagnostics()
            op.apply(case.dt, u, f)
    torch.cuda.synchronize()
    return op, (f.cpu().numpy() if f is not None else None), (out.cpu().numpy() if out is not None else None)


class _CourantFrom:
    """an oracle whose Courant diagnostics are another oracle's"""

    def __init__(self, orc, courant):
        self._orc, self._courant = orc, courant

    def diagnostics(self):
        return self._courant.diagnostics()

    def __getattr__(self, name):
        return getattr(self._orc, name)


def run_oracle(case, f0=None, ggrad=None):
    """F of the oracle (accumulated onto f0 if given) and the oracle to check the rest against.  Second order with ghost
    cells: the HIP scheme solves the cut edges on both ranks (all_edges_local: the owned rows of F are complete without the
    reverse exchange) while the Courant number is the owned edges' (edges.is_owned), as the reference's"""
    if ggrad is None:
        orc = oracle_from_case(case)
        return orc.apply(case.dt, case.u_local, None if f0 is None else f0.copy()), orc
    orcs = [oracle_from_case(case, all_edges_local=True), oracle_from_case(case)]
    for o in orcs:
        o.compute_gradients(case.u_local)
        for k in range(3):
            o.gradients[k][ggrad[0]] = ggrad[1][:, 2 * k:2 * k + 2]
        o.set_gradients_ready(True)
    fr = orcs[0].apply(case.dt, case.u_local, None if f0 is None else f0.copy())
    orcs[1].apply(case.dt, case.u_local, None if f0 is None else f0.copy())
    return fr, _CourantFrom(orcs[0], orcs[1])


def check_classes(case, f_gpu, f_ref, what):
    """the bar on each class of cell of the generator, normalised by the class's own maximum"""
    kind = case.cell_kind[case.mesh.cell_owned_to_local]
    for k, name in KIND_NAMES.items():
        sel = kind == k
        if sel.any():
            err = rel_linf(f_gpu[sel], f_ref[sel])
            assert err <= TOL, f"{what}: {name} cells ({sel.sum()}): rel L-inf {err:.3e}"


def check_against_oracle(case, call, op, f, out, fr, orc):
    """everything an evaluation leaves, against the oracle's"""
    mesh = case.mesh
    own = mesh.cell_owned_to_local
    assert np.isfinite(fr).all()
    if call == "euler":
        u = case.u_local
        assert np.all(out[mesh.cell_is_owned == 0] == -7.0), "ghost rows of u_out were written"
        err = rel_linf(out[own], u[own] + case.dt * fr)
        assert err <= TOL, f"u_out vs u + dt F_oracle: rel L-inf {err:.3e}"
        fe = (out[own] - u[own]) / case.dt
        check_all(case, fe, fr, op, orc)
        check_classes(case, fe, fr, "(u_out - u) / dt")
        if f is not None:
            assert rel_linf(f, fr) <= TOL
            check_classes(case, f, fr, "F of the Euler step")
    else:
        check_all(case, f, fr, op, orc)
        check_classes(case, f, fr, "F")
    err = rel_linf(op.flux_divergence.cpu().numpy(), orc.flux_divergence)
    assert err <= TOL, f"flux divergence: rel L-inf {err:.3e}"


# ---- part 1: one oracle comparison per instantiation ------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_instantiation_against_the_oracle(row, rdyhip_kernel, monkeypatch):
    if (rdyhip_kernel == "cell") != (row.kernel[0] == "cell"):
        pytest.skip("a row of the other kernel variant (RDYHIP_KERNEL)")
    assert row_kernel(row) == row.kernel
    if row.uout_cached is None:
        monkeypatch.delenv("RDYHIP_UOUT_CACHED", raising=False)
    else:
        monkeypatch.setenv("RDYHIP_UOUT_CACHED", str(row.uout_cached))
    rng = np.random.default_rng(5000 + ROWS.index(row))
    mesh = matrix_mesh(row.mesh, row.layout, row.well_balancing == 2)
    assert (mesh.num_owned_cells < mesh.num_cells) == (row.layout == "o2l")
    cfg = RDyFlowConfig(tiny_h=float(rng.choice([1e-7, 1e-5])), h_anuga_regular=float(rng.choice([0.0, 0.0, 1e-3])),
                        source_method=row.source_method, well_balancing=row.well_balancing, second_order=row.second_order,
                        limiter=row.limiter, cached_f_stores=row.cached_f_stores)
    case = random_case(rng, mesh, cfg, region_block=int(rng.choice([0, 32, 256])))
    f0 = rng.normal(size=(mesh.num_owned_cells, 3)) * np.array([0.1, 1.0, 1.0]) if row.call == "apply" else None
    ggrad = ghost_gradients(rng, case)
    with_f = row.call != "euler" or bool(rng.integers(0, 2))
    op, f, out = run_device(case, row.call, row.phased, f0=f0, with_f=with_f, ggrad=ggrad)
    info = op.layout_info()
    assert info["slots_per_cell"] == row.kernel[1] and info["owned_is_prefix"] == (row.layout == "prefix")
    assert info["tiled_kernel"] == (row.kernel[0] != "cell") and info["num_tiles"] >= (4 if row.kernel[0] != "cell" else 0)
    fr, orc = run_oracle(case, f0, ggrad)
    check_against_oracle(case, row.call, op, f, out, fr, orc)
    op.destroy()


# ---- part 2: the persistent tile walk ---------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class WalkCase:
    name: str
    kind: str                 # tri | quad | mixed
    nx: int
    ny: int
    seed: int
    tile_cells: int           # RDYHIP_TILE_CELLS of the case (the default run takes the default, 256)
    partition: bool           # one rank's part with interleaved ghosts: phased INTERIOR / HALO calls
    num_tiles: tuple          # (first order and HR, second order) at tile_cells: pinned by test_kernel_matrix_cpu.py
    knobs: tuple              # names in KNOBS


# every run of a case sets its tile_cells; RDYHIP_PGRID 8: one workgroup per XCD walks the XCD's whole chunk
KNOBS = {
    "g8":              {"RDYHIP_PGRID": "8"},
    "g8_flat_bal":     {"RDYHIP_PGRID": "8", "RDYHIP_XCD_SWIZZLE": "0", "RDYHIP_BALANCE_ROUNDS": "1"},
    "g24_bal":         {"RDYHIP_PGRID": "24", "RDYHIP_BALANCE_ROUNDS": "1"},
    "g24_flat":        {"RDYHIP_PGRID": "24", "RDYHIP_XCD_SWIZZLE": "0"},
    "g24_shrink2":     {"RDYHIP_PGRID": "24", "RDYHIP_INTERIOR_SHRINK": "2"},
    "g8_shrink2_bal":  {"RDYHIP_PGRID": "8", "RDYHIP_INTERIOR_SHRINK": "2", "RDYHIP_BALANCE_ROUNDS": "1"},
}
_KNOB_VARS = ("RDYHIP_PGRID", "RDYHIP_XCD_SWIZZLE", "RDYHIP_BALANCE_ROUNDS", "RDYHIP_INTERIOR_SHRINK", "RDYHIP_TILE_CELLS",
              "RDYHIP_UOUT_CACHED", "RDYHIP_BLOCKS_PER_CU")

WALK_CASES = [
    # below 64 tiles: no XCD chunks, the grid strides over the tiles
    WalkCase("tri_lt64", "tri", 20, 375, 21, 256, False, (59, 59), ("g8", "g24_flat")),
    # exactly 64 tiles: the smallest chunked walk, 8 tiles per XCD
    WalkCase("quad_64", "quad", 16, 946, 22, 256, False, (64, 64), ("g8", "g24_bal", "g8_flat_bal")),
    # num_tiles % 8 == 1: the last XCD's chunk is one tile long
    WalkCase("mixed_mod1", "mixed", 50, 318, 23, 64, False, (377, 457), ("g8", "g24_bal")),
    # a multiple of 8: every chunk full
    WalkCase("quad_mult8", "quad", 64, 402, 24, 64, False, (536, 801), ("g24_flat", "g8_flat_bal")),
    # num_tiles % 8 == 7, a part with interleaved ghosts: INTERIOR tiles skipped in the chunks, the shrunken INTERIOR grid
    WalkCase("tri_part_mod7", "tri", 48, 326, 25, 256, True, (71, 71), ("g8", "g24_shrink2", "g8_shrink2_bal")),
]


@functools.lru_cache(maxsize=None)
def walk_mesh(name, project_2d):
    c = next(w for w in WALK_CASES if w.name == name)
    rng = np.random.default_rng(c.seed)
    if c.partition:
        return random_partition_mesh(rng, c.kind, c.nx, c.ny, project_2d=project_2d)
    return random_mesh(rng, c.kind, c.nx, c.ny, project_2d=project_2d, permute=False)


WALK_VARIANTS = {"first": (0, False, MM), "hr": (2, False, MM), "second_minmod": (0, True, MM), "second_vanleer": (0, True, VL)}


def _set_knobs(monkeypatch, env):
    for k in _KNOB_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("variant", list(WALK_VARIANTS))
@pytest.mark.parametrize("wc", WALK_CASES, ids=[w.name for w in WALK_CASES])
def test_tile_walk_against_the_oracle_and_the_default_walk(wc, variant, rdyhip_kernel, monkeypatch):
    if rdyhip_kernel == "cell":
        pytest.skip("tiled kernels only")
    wb, so, lim = WALK_VARIANTS[variant]
    mesh = walk_mesh(wc.name, wb == 2)
    rng = np.random.default_rng(wc.seed * 10 + list(WALK_VARIANTS).index(variant))
    cfg = RDyFlowConfig(tiny_h=1e-5, h_anuga_regular=float(rng.choice([0.0, 1e-3])), source_method=int(rng.integers(0, 2)),
                        well_balancing=wb, second_order=so, limiter=lim)
    case = random_case(rng, mesh, cfg, region_block=wc.tile_cells)
    case.dt = 1e-2
    ggrad = ghost_gradients(rng, case)
    fr, orc = run_oracle(case, ggrad=ggrad)
    for call in ("rhs", "euler"):
        _set_knobs(monkeypatch, {})
        op, f, out = run_device(case, call, wc.partition, ggrad=ggrad)
        check_against_oracle(case, call, op, f, out, fr, orc)
        op.update_diagnostics()
        d0 = op.get_diagnostics()
        op.destroy()
        for name in wc.knobs:
            _set_knobs(monkeypatch, dict(KNOBS[name], RDYHIP_TILE_CELLS=str(wc.tile_cells)))
            op, f2, out2 = run_device(case, call, wc.partition, ggrad=ggrad)
            info = op.layout_info()
            assert info["num_tiles"] == wc.num_tiles[1 if so else 0]
            assert info["persistent_grid"] == int(KNOBS[name]["RDYHIP_PGRID"])
            check_against_oracle(case, call, op, f2, out2, fr, orc)
            op.update_diagnostics()
            d = op.get_diagnostics()
            assert (d.max_courant_num, d.global_edge_id, d.global_cell_id) == (d0.max_courant_num, d0.global_edge_id, d0.global_cell_id), name
            assert np.array_equal(f2, f), f"{name}: F differs from the default walk's"
            if call == "euler":
                assert np.array_equal(out2, out), f"{name}: u_out differs from the default walk's"
            op.destroy()
