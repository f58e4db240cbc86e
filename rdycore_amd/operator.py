"""Host-side mirror of RDycore's Operator interface for the SWE right-hand side.

Same names, argument meaning and error behaviour as the reference's
`CreateOperator / ApplyOperator / DestroyOperator` boundary and its data
setters (include/private/rdyoperatorimpl.h:208-271, src/operator.c), on top of
the C ABI in include/rdyhip.h.  torch is used only for device memory and
streams: `u_local` / `f_global` are float64 CUDA tensors laid out like the
PETSc Vecs they stand for ([num_cells,3] local, [num_owned_cells,3] global).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import RDyHipError  # noqa: F401  (re-export)
from .mesh import (CONDITION_CRITICAL_OUTFLOW, CONDITION_DIRICHLET, CONDITION_REFLECTING, RDyMesh)

SOURCE_SEMI_IMPLICIT = 0     # RDyFlowSourceMethod, include/private/rdyconfigimpl.h:52-56
SOURCE_IMPLICIT_XQ2018 = 1
RIEMANN_ROE = 0
WELL_BALANCING_NONE = 0      # RDyWellBalanceMethod, include/private/rdyconfigimpl.h:58-62
WELL_BALANCING_HR = 2        # hydrostatic reconstruction
LIMITER_MINMOD, LIMITER_NONE, LIMITER_VANLEER = 0, 1, 2   # RDyLimiterType, include/private/rdyconfigimpl.h:64-71

PHASE_ALL, PHASE_INTERIOR, PHASE_HALO = 0, 1, 2
OUTPUT_SOLUTION, OUTPUT_PRIMITIVE_VARIABLES, OUTPUT_SOURCES = 1, 2, 4   # RDYHIP_OUTPUT_*: the time-averaged output fields
SERIES_OBSERVATIONS, SERIES_BOUNDARY_FLUXES = 1, 2                      # RDYHIP_SERIES_*: the time series kept on the device
COMPONENT_H, COMPONENT_HU, COMPONENT_HV = 1, 2, 4                       # RDYHIP_COMPONENT_*: the planes of the state read-out
MAX_TRACERS = 7                                                         # RDYHIP_MAX_TRACERS
TRACER_RIEMANN_ROE, TRACER_RIEMANN_UPWIND_ROE = 0, 1                    # RDYHIP_TRACER_RIEMANN_*
TRACER_FORM_CONSERVED, TRACER_FORM_PRIMITIVE = 0, 1                     # RDYHIP_TRACER_FORM_*: the rows of the tracer read-out
DIAGNOSTICS_OPERATOR, DIAGNOSTICS_ENSEMBLE = 0, 1                       # RDYHIP_DIAGNOSTICS_*: the scopes of the non-blocking read-back


@dataclasses.dataclass
class RDyFlowConfig:
    """The scalars of RDyConfig that reach the SWE operator, with the defaults
    of src/yaml_input.c:851-865."""
    tiny_h: float = 1e-7
    h_anuga_regular: float = 0.0
    xq2018_threshold: float = 1e-10
    source_method: int = SOURCE_SEMI_IMPLICIT
    riemann: int = RIEMANN_ROE
    well_balancing: int = WELL_BALANCING_NONE
    second_order: bool = False        # numerics.second_order: MUSCL reconstruction (src/swe/swe_petsc.c:98-213)
    limiter: int = LIMITER_MINMOD     # numerics.limiter
    cached_f_stores: bool = False     # RDYHIP_CONFIG_CACHED_F_STORES: F is read back by a separate update kernel (TSEULER's VecAXPY)
    streamed_normals: bool = False    # RDYHIP_CONFIG_STREAMED_NORMALS: no normal table, whatever the mesh (tests, A/B timings)


@dataclasses.dataclass
class CourantNumberDiagnostics:
    """include/private/rdyoperatorimpl.h:21-25"""
    max_courant_num: float
    global_edge_id: int
    global_cell_id: int


class _DeviceArray:
    """Wraps a raw device pointer for torch.as_tensor (zero copy)."""

    def __init__(self, ptr: int, shape: Tuple[int, ...], owner):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (ptr, False), "version": 2}


def _ptr(t) -> int:
    return int(t.data_ptr())


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _abi_arguments(config: "RDyFlowConfig", mesh: RDyMesh, condition_types: Optional[Sequence[int]]):
    """RDyHipConfig / RDyHipMesh / RDyHipBoundary[] for a mesh (the arrays are borrowed: keep `keep` alive during the call)"""
    nb = len(mesh.boundaries)
    if condition_types is None:
        condition_types = [CONDITION_REFLECTING] * nb
    if len(condition_types) != nb:
        raise RDyHipError(83, f"{len(condition_types)} boundary conditions for {nb} boundaries")
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a

    m = _lib.RDyHipMesh()
    m.num_cells, m.num_owned_cells = mesh.num_cells, mesh.num_owned_cells
    m.num_edges, m.num_internal_edges = mesh.num_edges, mesh.num_internal_edges
    m.cell_is_owned = arr(mesh.cell_is_owned, np.int32).ctypes.data_as(_lib.c_int32_p)
    m.cell_local_to_owned = arr(mesh.cell_local_to_owned, np.int32).ctypes.data_as(_lib.c_int32_p)
    m.cell_global_ids = arr(mesh.cell_global_ids, np.int64).ctypes.data_as(_lib.c_int64_p)
    m.cell_areas = arr(mesh.cell_areas, np.float64).ctypes.data_as(_lib.c_double_p)
    m.cell_dz_dx = arr(mesh.cell_dz_dx, np.float64).ctypes.data_as(_lib.c_double_p)
    m.cell_dz_dy = arr(mesh.cell_dz_dy, np.float64).ctypes.data_as(_lib.c_double_p)
    m.edge_cell_ids = arr(mesh.edge_cell_ids, np.int32).ctypes.data_as(_lib.c_int32_p)
    m.edge_internal_ids = arr(mesh.edge_internal_ids, np.int32).ctypes.data_as(_lib.c_int32_p)
    m.edge_global_ids = arr(mesh.edge_global_ids, np.int64).ctypes.data_as(_lib.c_int64_p)
    m.edge_lengths = arr(mesh.edge_lengths, np.float64).ctypes.data_as(_lib.c_double_p)
    m.edge_cn = arr(mesh.edge_cn, np.float64).ctypes.data_as(_lib.c_double_p)
    m.edge_sn = arr(mesh.edge_sn, np.float64).ctypes.data_as(_lib.c_double_p)
    m.cell_zc = arr(mesh.cell_zc, np.float64).ctypes.data_as(_lib.c_double_p)
    if config.second_order:
        m.num_vertices = mesh.num_vertices
        m.cell_centroids = arr(mesh.cell_centroids, np.float64).ctypes.data_as(_lib.c_double_p)
        m.edge_vertex_ids = arr(mesh.edge_vertex_ids, np.int32).ctypes.data_as(_lib.c_int32_p)
        m.vertex_points = arr(mesh.xyz, np.float64).ctypes.data_as(_lib.c_double_p)
        if mesh.num_cells > mesh.num_owned_cells:      # edges.is_owned: who reports the Courant number of a cut edge (swe_petsc.c:172-190)
            m.edge_is_owned = arr(mesh.edge_is_owned(), np.int32).ctypes.data_as(_lib.c_int32_p)
    barr = (_lib.RDyHipBoundary * max(nb, 1))()
    for i, b in enumerate(mesh.boundaries):
        barr[i].num_edges = b.num_edges
        barr[i].edge_ids = arr(b.edge_ids, np.int32).ctypes.data_as(_lib.c_int32_p)
        barr[i].condition_type = int(condition_types[i])
    cfg = _lib.RDyHipConfig(config.tiny_h, config.h_anuga_regular, config.xq2018_threshold,
                            int(config.source_method), int(config.riemann), int(config.well_balancing),
                            1 if config.second_order else 0, int(config.limiter),
                            (1 if getattr(config, "cached_f_stores", False) else 0) | (2 if getattr(config, "streamed_normals", False) else 0))
    return cfg, m, nb, barr, list(condition_types), keep


def probe_layout(config: "RDyFlowConfig", mesh: RDyMesh, condition_types: Optional[Sequence[int]] = None) -> dict:
    """rdyhip_probe_layout: the host-side layout pass of rdyhip_create alone (no GPU needed) -- validates the mesh
    exactly as create does and returns the layout numbers (tiles, edge records, halo lists, LDS per workgroup)."""
    cfg, m, nb, barr, _, _keep = _abi_arguments(config, mesh, condition_types)
    info = _lib.RDyHipLayoutInfo()
    _lib.check(_lib.load().rdyhip_probe_layout(C.byref(cfg), C.byref(m), nb, barr, C.byref(info)))
    return {k: getattr(info, k) for k, _ in info._fields_}


def plan_series_boundary_edges(mesh: RDyMesh, boundaries=None):
    """rdyhip_series_plan_boundary_edges: which boundary edges a boundary-flux record of `mesh` holds -- (local edge id,
    boundary) per row, in record order -- for the listed boundaries (None: all).  Host only, no device needed."""
    cfg, m, nb, barr, _, _keep = _abi_arguments(RDyFlowConfig(), mesh, None)
    room = max(sum(b.num_edges for b in mesh.boundaries), 1)
    e, b = np.zeros(room, dtype=np.int32), np.zeros(room, dtype=np.int32)
    n = C.c_int32()
    if boundaries is None:
        nl, lp = 0, None
    else:
        listed = np.ascontiguousarray(boundaries, dtype=np.int32).ravel()
        arg = listed if listed.size else np.zeros(1, dtype=np.int32)
        nl, lp = int(listed.size), arg.ctypes.data_as(_lib.c_int32_p)
    _lib.check(_lib.load().rdyhip_series_plan_boundary_edges(C.byref(m), nb, barr, nl, lp, C.byref(n), e.ctypes.data_as(_lib.c_int32_p),
                                                            b.ctypes.data_as(_lib.c_int32_p)))
    return e[:n.value].copy(), b[:n.value].copy()


UNIFORM_SOURCE, UNIFORM_MANNINGS, UNIFORM_FLAT_BED = 1, 2, 4   # bits of Operator.uniform_fields()


class Operator:
    """Operator (include/private/rdyoperatorimpl.h:103-201), native MI355X backend."""

    def __init__(self, handle, mesh: RDyMesh, config: RDyFlowConfig, condition_types: Sequence[int]):
        self._h = handle
        self.mesh = mesh
        self.config = config
        self.condition_types = list(condition_types)
        self.num_components = 3

    # -- CreateOperator (src/operator.c:348-417) ---------------------------
    @classmethod
    def create(cls, config: RDyFlowConfig, mesh: RDyMesh, condition_types: Optional[Sequence[int]] = None) -> "Operator":
        """`condition_types[b]` is the flow condition type of `mesh.boundaries[b]`
        (a boundary with no condition is reflecting, src/rdysetup.c:283-503)."""
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("rdycore_amd.Operator needs a HIP device (no CPU fallback)")
        torch.cuda.current_device()  # make sure the HIP context exists on the chosen device
        cfg, m, nb, barr, condition_types, _keep = _abi_arguments(config, mesh, condition_types)
        h = C.c_void_p()
        _lib.check(lib.rdyhip_create(C.byref(cfg), C.byref(m), nb, barr, C.byref(h)))
        return cls(h, mesh, config, condition_types)

    # -- DestroyOperator (src/operator.c:421-493) --------------------------
    def destroy(self):
        if self._h is not None and self._h.value:
            _lib.check(_lib.load().rdyhip_destroy(C.byref(self._h)))
        self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # The state tensor of the most recent evaluation stays alive with the operator: while the primitive variables are not
    # stored, the first request for them reads it (rdyhip_field_ptr in include/rdyhip.h) -- a caller that drops its own
    # reference right after the call must not hand the memory back to the allocator.  In-place writes remain the caller's.
    _last_state = None

    # -- argument checks shared by the apply calls -------------------------
    def _check_vecs(self, u_local: torch.Tensor, f_global: torch.Tensor):
        for name, t, n in (("u_local", u_local, self.mesh.num_cells), ("f_global", f_global, self.mesh.num_owned_cells)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
                raise RDyHipError(83, f"{name} must be a contiguous float64 device tensor")
            if t.numel() != 3 * n:
                # src/swe/swe_petsc.c:234
                raise RDyHipError(83, f"Number of dof in {name} must be 3! ({t.numel()} values for {n} cells)")

    # -- ApplyOperator (src/operator.c:680-690): f_global += F(u_local) ----
    def apply(self, dt: float, u_local: torch.Tensor, f_global: torch.Tensor):
        self._check_vecs(u_local, f_global)
        self._last_state = u_local
        _lib.check(_lib.load().rdyhip_apply(self._h, float(dt), _ptr(u_local), _ptr(f_global), _stream()))

    # -- OperatorRHSFunction's zero + reset + apply (src/rdysetup.c:1130-1139), fused
    def rhs_function(self, dt: float, u_local: torch.Tensor, f_global: torch.Tensor):
        self._check_vecs(u_local, f_global)
        self._last_state = u_local
        _lib.check(_lib.load().rdyhip_rhs_function(self._h, float(dt), _ptr(u_local), _ptr(f_global), _stream()))

    def apply_phase(self, phase: int, overwrite: bool, dt: float, u_local: torch.Tensor, f_global: torch.Tensor,
                    reset_diagnostics: bool = False, gradients_ready: bool = False):
        self._check_vecs(u_local, f_global)
        flags = (1 if overwrite else 0) | (2 if reset_diagnostics else 0) | (4 if gradients_ready else 0)
        self._last_state = u_local
        _lib.check(_lib.load().rdyhip_apply_phase(self._h, int(phase), flags, float(dt), _ptr(u_local),
                                                 _ptr(f_global), _stream()))

    # -- TSStep_Euler fused with the RHS: u_out[owned] = u_local[owned] + dt * RHS(u_local) ----------------
    def euler_step(self, dt: float, u_local: torch.Tensor, u_out: torch.Tensor, f_global: Optional[torch.Tensor] = None,
                   phase: int = PHASE_ALL, reset_diagnostics: bool = True, gradients_ready: bool = False):
        """One forward-Euler step without a separate axpy pass (rdyhip_euler_step).  Not in place; the ghost rows
        of u_out are the next halo update's.  f_global=None: F is not stored at all where the kernel allows it."""
        n = self.mesh.num_cells
        for name, t in (("u_local", u_local), ("u_out", u_out)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == 3 * n):
                raise RDyHipError(83, f"{name} must be a contiguous float64 device tensor of {n} cells x 3")
        if f_global is not None:
            self._check_vecs(u_local, f_global)
        flags = (2 if reset_diagnostics else 0) | (4 if gradients_ready else 0)
        self._last_state = u_local
        _lib.check(_lib.load().rdyhip_euler_step(self._h, int(phase), flags, float(dt), _ptr(u_local), _ptr(u_out),
                                                 _ptr(f_global) if f_global is not None else None, _stream()))

    # -- TSStep_RK with the TSRK4 tableau (src/rdysetup.c:1187-1189): four stage evaluations, the stage vectors on the device --
    def rk4_step(self, dt: float, u_local: torch.Tensor, halo=None):
        """One classical Runge-Kutta step of u_local's owned rows, in place (rdyhip_rk4_step).  `halo`: the HaloExchange of
        a multi-rank run with the exchange behind the C ABI (transport="c"); None, or a halo of one rank: no ghost update.
        The stage vectors live in a workspace of the operator, allocated by the first call."""
        n = self.mesh.num_cells
        if not (isinstance(u_local, torch.Tensor) and u_local.is_cuda and u_local.dtype == torch.float64 and u_local.is_contiguous()
                and u_local.numel() == 3 * n):
            raise RDyHipError(83, f"u_local must be a contiguous float64 device tensor of {n} cells x 3")
        h = getattr(halo, "_halo", None) if halo is not None else None
        if halo is not None and h is None and getattr(halo, "world", 1) > 1:
            raise RDyHipError(83, 'rk4_step needs a halo with the exchange behind the C ABI (HaloExchange(transport="c"))')
        self._last_state = None      # the state of the last evaluation is the operator's own stage array
        _lib.check(_lib.load().rdyhip_rk4_step(self._h, h, float(dt), _ptr(u_local), _stream()))

    # -- time-averaged output fields (WriteXDMFOutput's OutputVars, src/xdmf_output.c:196-241, 436-504) ------------------
    def enable_output_means(self, vars: int):
        """rdyhip_output_mean_enable: a zeroed [owned,3] accumulator for each of OUTPUT_SOLUTION | OUTPUT_PRIMITIVE_VARIABLES |
        OUTPUT_SOURCES in `vars` that has none yet."""
        _lib.check(_lib.load().rdyhip_output_mean_enable(self._h, int(vars)))

    def accumulate_output_means(self, vars: int, dt: float, u_local: Optional[torch.Tensor] = None):
        """AccumulateOutputVar for all of `vars` in one launch on the current stream (rdyhip_output_mean_accumulate): the
        solution from `u_local` ([num_cells,3], needed only with OUTPUT_SOLUTION), the primitive variables of the most recent
        evaluation and the operator's source array; the evaluations go on not storing the primitive variables."""
        if u_local is not None:
            n = self.mesh.num_cells
            if not (isinstance(u_local, torch.Tensor) and u_local.is_cuda and u_local.dtype == torch.float64 and u_local.is_contiguous()
                    and u_local.numel() == 3 * n):
                raise RDyHipError(83, f"u_local must be a contiguous float64 device tensor of {n} cells x 3")
        _lib.check(_lib.load().rdyhip_output_mean_accumulate(self._h, int(vars), float(dt), _ptr(u_local) if u_local is not None else None,
                                                            _stream()))

    def output_mean(self, var: int):
        """ComputeMean of one variable (rdyhip_output_mean_get): (mean [owned,3], accumulated time); nothing is reset."""
        out = torch.empty((self.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
        t = C.c_double()
        _lib.check(_lib.load().rdyhip_output_mean_get(self._h, int(var), _ptr(out), C.byref(t), _stream()))
        return out, t.value

    def reset_output_means(self, vars: int):
        """ResetOutputVar (rdyhip_output_mean_reset): accumulators and times of `vars` back to zero, on the current stream"""
        _lib.check(_lib.load().rdyhip_output_mean_reset(self._h, int(vars), _stream()))

    def output_mean_time(self, var: int) -> float:
        t = C.c_double()
        _lib.check(_lib.load().rdyhip_output_mean_time(self._h, int(var), C.byref(t)))
        return t.value

    # -- time series on the device (WriteTimeSeries, src/time_series.c:530-564) -----------------------------------------------
    def enable_observation_series(self, owned_cell_ids, capacity: int):
        """rdyhip_series_observations_enable (InitObservations): a device log of `capacity` records of the state in the cells
        `owned_cell_ids` (owned-cell indices; a site may repeat)"""
        ids = np.ascontiguousarray(owned_cell_ids, dtype=np.int32).ravel()
        arg = ids if ids.size else np.zeros(1, dtype=np.int32)
        _lib.check(_lib.load().rdyhip_series_observations_enable(self._h, int(ids.size), arg.ctypes.data_as(_lib.c_int32_p), int(capacity)))

    def enable_boundary_flux_series(self, capacity: int, boundaries=None):
        """rdyhip_series_boundary_fluxes_enable (InitBoundaryFluxes): a device log of `capacity` records with one row per boundary
        edge of `boundaries` (indices; None: all) whose left cell is owned"""
        if boundaries is None:
            _lib.check(_lib.load().rdyhip_series_boundary_fluxes_enable(self._h, 0, None, int(capacity)))
            return
        b = np.ascontiguousarray(boundaries, dtype=np.int32).ravel()
        arg = b if b.size else np.zeros(1, dtype=np.int32)      # an empty list is a list, not "all"
        _lib.check(_lib.load().rdyhip_series_boundary_fluxes_enable(self._h, int(b.size), arg.ctypes.data_as(_lib.c_int32_p), int(capacity)))

    def series_boundary_edges(self):
        """rdyhip_series_boundary_edges: (local edge id, boundary) of every row of a boundary-flux record, in record order"""
        n = C.c_int32()
        e, b = _lib.c_int32_p(), _lib.c_int32_p()
        _lib.check(_lib.load().rdyhip_series_boundary_edges(self._h, C.byref(n), C.byref(e), C.byref(b)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(e, (n.value,)).copy(), np.ctypeslib.as_array(b, (n.value,)).copy()

    def series_add_time(self, dt: float):
        """AccumulateBoundaryFluxes (rdyhip_series_boundary_fluxes_add_time): accumulated_time += dt"""
        _lib.check(_lib.load().rdyhip_series_boundary_fluxes_add_time(self._h, float(dt)))

    def series_record(self, kind: int, time: float, u_local: Optional[torch.Tensor] = None):
        """rdyhip_series_record: one record of SERIES_OBSERVATIONS (the state `u_local`, [num_cells,3]) or SERIES_BOUNDARY_FLUXES
        appended to its device log, one launch on the current stream"""
        if u_local is not None:
            n = self.mesh.num_cells
            if not (isinstance(u_local, torch.Tensor) and u_local.is_cuda and u_local.dtype == torch.float64 and u_local.is_contiguous()
                    and u_local.numel() == 3 * n):
                raise RDyHipError(83, f"u_local must be a contiguous float64 device tensor of {n} cells x 3")
        _lib.check(_lib.load().rdyhip_series_record(self._h, int(kind), float(time), _ptr(u_local) if u_local is not None else None, _stream()))

    def series_info(self, kind: int) -> dict:
        """rdyhip_series_info: rows of a record, records in the log, capacity, accumulated time"""
        e, n, cap, t = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        _lib.check(_lib.load().rdyhip_series_info(self._h, int(kind), C.byref(e), C.byref(n), C.byref(cap), C.byref(t)))
        return {"entries": e.value, "count": n.value, "capacity": cap.value, "accumulated_time": t.value}

    def series_read(self, kind: int, first: int = 0, count: Optional[int] = None):
        """rdyhip_series_read: (times [count], values [count, entries, 3]) of records [first, first + count) as numpy arrays
        (count=None: all from `first`); synchronises the current stream"""
        info = self.series_info(kind)
        if count is None:
            count = max(info["count"] - int(first), 0)
        times = np.zeros(max(int(count), 0))
        values = np.zeros((max(int(count), 0), info["entries"], 3))
        tp = times.ctypes.data_as(_lib.c_double_p) if times.size else None
        vp = values.ctypes.data_as(_lib.c_double_p) if values.size else None
        _lib.check(_lib.load().rdyhip_series_read(self._h, int(kind), int(first), int(count), tp, vp, _stream()))
        return times, values

    def series_device_log(self, kind: int) -> torch.Tensor:
        """rdyhip_series_device_log: the whole log as a [capacity, entries, 3] device tensor, no copy"""
        p = C.c_void_p()
        _lib.check(_lib.load().rdyhip_series_device_log(self._h, int(kind), C.byref(p)))
        info = self.series_info(kind)
        shape = (info["capacity"], info["entries"], 3)
        if shape[0] * shape[1] == 0:
            return torch.zeros(shape, dtype=torch.float64, device="cuda")
        return torch.as_tensor(_DeviceArray(p.value, (shape[0] * shape[1] * 3,), self), device="cuda").view(shape)

    def series_clear(self, kind: int):
        """rdyhip_series_clear: the log holds no records; the accumulated time of the boundary series stays"""
        _lib.check(_lib.load().rdyhip_series_clear(self._h, int(kind)))

    # -- state read-out: RDyGetOwnedCell{Heights,XMomenta,YMomenta} (src/rdydata.c:171-205), RDyMMSComputeErrorNorms (src/rdymms.c:850-903)
    def _check_state(self, u_local, name="u_local", cells=None):
        n = self.mesh.num_cells if cells is None else cells
        if not (isinstance(u_local, torch.Tensor) and u_local.is_cuda and u_local.dtype == torch.float64 and u_local.is_contiguous()
                and u_local.numel() == 3 * n):
            raise RDyHipError(83, f"{name} must be a contiguous float64 device tensor of {n} cells x 3")

    def state_planes(self, u_local: torch.Tensor, comps: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """rdyhip_state_planes: [popcount(comps), owned] device tensor, plane k = the k-th component of COMPONENT_H | COMPONENT_HU |
        COMPONENT_HV in `comps` (ascending) of the owned cells, bit for bit; one launch on the current stream.  `out`: a
        contiguous float64 device tensor with room for the planes, written from its start."""
        self._check_state(u_local)
        k = bin(int(comps) & 7).count("1") if 1 <= int(comps) <= 7 else 0
        no = self.mesh.num_owned_cells
        if out is None:
            out = torch.empty((k, no), dtype=torch.float64, device="cuda")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= k * no):
            raise RDyHipError(83, f"out must be a contiguous float64 device tensor of at least {k} x {no} values")
        _lib.check(_lib.load().rdyhip_state_planes(self._h, int(comps), _ptr(u_local), _ptr(out), _stream()))
        return out

    def read_state_begin(self, u_local: torch.Tensor, comps: int):
        """rdyhip_state_read_begin: de-interleave `comps` of the owned cells on the current stream and start their copy to pinned
        host memory on the operator's copy stream; returns at once.  u_local is read at this place in the stream."""
        self._check_state(u_local)
        _lib.check(_lib.load().rdyhip_state_read_begin(self._h, int(comps), _ptr(u_local), _stream()))

    def read_state_ready(self) -> bool:
        """rdyhip_state_read_ready: the copy of the last read_state_begin has finished (an event query)"""
        out = C.c_int32()
        _lib.check(_lib.load().rdyhip_state_read_ready(self._h, C.byref(out)))
        return bool(out.value)

    def read_state(self, comp: int) -> np.ndarray:
        """rdyhip_state_read_wait + rdyhip_state_read_get: waits for the copy of the last read_state_begin (for that alone) and
        returns component `comp` (exactly one COMPONENT_*) of the owned cells as a numpy array"""
        lib = _lib.load()
        _lib.check(lib.rdyhip_state_read_wait(self._h))
        out = np.empty(self.mesh.num_owned_cells)
        _lib.check(lib.rdyhip_state_read_get(self._h, int(comp), int(out.size), out.ctypes.data_as(_lib.c_double_p) if out.size else None))
        return out

    def error_sums(self, u_local: torch.Tensor, exact: Optional[torch.Tensor] = None) -> dict:
        """rdyhip_error_sums + rdyhip_error_sums_get: {"l1", "l2_squared", "linf": [3] arrays, "area": float} of u_local - exact over
        the owned cells of this rank (`exact`: [owned,3] device tensor; None: zeros, so l1[0] is the water volume); the reduction
        over ranks and the square root of RDyMMSComputeErrorNorms are the caller's"""
        self._check_state(u_local)
        if exact is not None:
            self._check_state(exact, "exact", self.mesh.num_owned_cells)
        lib = _lib.load()
        _lib.check(lib.rdyhip_error_sums(self._h, _ptr(u_local), _ptr(exact) if exact is not None else None, _stream()))
        s = _lib.RDyHipErrorSums()
        _lib.check(lib.rdyhip_error_sums_get(self._h, C.byref(s)))
        return {"l1": np.array(s.l1[:]), "l2_squared": np.array(s.l2_squared[:]), "linf": np.array(s.linf[:]), "area": float(s.area)}

    # -- shallow water with advected tracers (src/tracer/tracer_petsc.c): state [num_cells, 3 + NT] = (h, hu, hv, h c_0 ...) --------
    num_tracers = 0

    def enable_tracers(self, n: int, riemann: int = TRACER_RIEMANN_ROE, well_balancing: int = WELL_BALANCING_NONE):
        """rdyhip_tracers_enable: the tracer path with `n` tracers (1..7) and the Roe (0) or upwind Roe (1) tracer flux; allocates
        its boundary values / fluxes [K, 3 + n] and tracer sources [owned, n], all zero.  well_balancing=WELL_BALANCING_HR:
        rdyhip_tracer_hr_enable, the same on an operator created with hydrostatic reconstruction (every tracer call then
        evaluates the HR form); the default refuses such an operator."""
        if well_balancing == WELL_BALANCING_HR:
            _lib.check(_lib.load().rdyhip_tracer_hr_enable(self._h, int(n), int(riemann)))
        elif well_balancing == WELL_BALANCING_NONE:
            _lib.check(_lib.load().rdyhip_tracers_enable(self._h, int(n), int(riemann)))
        else:
            raise ValueError(f"well_balancing is WELL_BALANCING_NONE or WELL_BALANCING_HR, not {well_balancing}")
        self.num_tracers = int(n)

    def tracers_well_balancing(self) -> int:
        """rdyhip_tracer_hr_info: WELL_BALANCING_HR after enable_tracers(..., well_balancing=WELL_BALANCING_HR), else WELL_BALANCING_NONE"""
        wb = C.c_int32()
        _lib.check(_lib.load().rdyhip_tracer_hr_info(self._h, C.byref(wb)))
        return wb.value

    def tracers_info(self) -> Tuple[int, int]:
        """rdyhip_tracers_info: (number of tracers -- 0: not enabled --, tracer Riemann solver)"""
        n, r = C.c_int32(), C.c_int32()
        _lib.check(_lib.load().rdyhip_tracers_info(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def _check_tracer_state(self, t, name: str, cells: int, optional: bool = False):
        if optional and t is None:
            return
        n = 3 + self.num_tracers
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n * cells):
            raise RDyHipError(83, f"{name} must be a contiguous float64 device tensor of {cells} cells x {n}")

    def tracers_set_boundary_values(self, boundary: int, values):
        """values[e, :] = (h, hu, hv, h c_0 ...) of boundary edge e, all 3 + NT components (rdyhip_tracers_set_boundary_values)"""
        v = np.ascontiguousarray(values, dtype=np.float64)
        ne = v.shape[0] if v.ndim == 2 and v.shape[1] == 3 + self.num_tracers else -1
        _lib.check(_lib.load().rdyhip_tracers_set_boundary_values(self._h, int(boundary), int(ne), v.ctypes.data_as(_lib.c_double_p) if v.size else None))

    def tracers_set_source(self, tracer: int, values, owned_cell_ids=None):
        """rdyhip_tracers_set_source: the source of tracer `tracer` in the owned cells `owned_cell_ids` (None: cells 0 .. n - 1)"""
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        ip = None
        if owned_cell_ids is not None:
            ids = np.ascontiguousarray(owned_cell_ids, dtype=np.int32).ravel()
            if ids.size != v.size:
                raise RDyHipError(60, f"size ({v.size}) does not match the region size ({ids.size})")
            ip = ids.ctypes.data_as(_lib.c_int32_p)
        _lib.check(_lib.load().rdyhip_tracers_set_source(self._h, int(tracer), int(v.size), ip, v.ctypes.data_as(_lib.c_double_p) if v.size else None))

    def tracers_rhs_function(self, dt: float, u_local: torch.Tensor, f_global: torch.Tensor):
        """rdyhip_tracers_rhs_function: f_global [owned, 3 + NT] = F(u_local [num_cells, 3 + NT]), diagnostics reset, one launch"""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        self._check_tracer_state(f_global, "f_global", self.mesh.num_owned_cells)
        _lib.check(_lib.load().rdyhip_tracers_rhs_function(self._h, float(dt), _ptr(u_local), _ptr(f_global), _stream()))

    def tracers_euler_step(self, dt: float, u_local: torch.Tensor, u_out: torch.Tensor, f_global: Optional[torch.Tensor] = None):
        """rdyhip_tracers_euler_step: u_out[owned rows] = fma(dt, F, u_local), not in place; f_global=None: F is never stored"""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        self._check_tracer_state(u_out, "u_out", self.mesh.num_cells)
        self._check_tracer_state(f_global, "f_global", self.mesh.num_owned_cells, optional=True)
        _lib.check(_lib.load().rdyhip_tracers_euler_step(self._h, float(dt), _ptr(u_local), _ptr(u_out),
                                                         _ptr(f_global) if f_global is not None else None, _stream()))

    def tracers_rhs_phase(self, phase: int, dt: float, u_local: torch.Tensor, f_global: torch.Tensor, reset_diagnostics: bool = False):
        """rdyhip_tracer_phase_rhs: tracers_rhs_function for the owned cells of one phase (0: all, 1: without a ghost neighbour,
        2: with one); rows of the other phase are not touched.  reset_diagnostics=False merges into the Courant diagnostic"""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        self._check_tracer_state(f_global, "f_global", self.mesh.num_owned_cells)
        _lib.check(_lib.load().rdyhip_tracer_phase_rhs(self._h, int(phase), 2 if reset_diagnostics else 0, float(dt), _ptr(u_local), _ptr(f_global),
                                                       _stream()))

    def tracers_euler_step_phase(self, phase: int, dt: float, u_local: torch.Tensor, u_out: torch.Tensor, f_global: Optional[torch.Tensor] = None,
                                 reset_diagnostics: bool = False):
        """rdyhip_tracer_phase_euler_step: tracers_euler_step for the owned cells of one phase, each phase writing its own rows of
        u_out"""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        self._check_tracer_state(u_out, "u_out", self.mesh.num_cells)
        self._check_tracer_state(f_global, "f_global", self.mesh.num_owned_cells, optional=True)
        _lib.check(_lib.load().rdyhip_tracer_phase_euler_step(self._h, int(phase), 2 if reset_diagnostics else 0, float(dt), _ptr(u_local), _ptr(u_out),
                                                              _ptr(f_global) if f_global is not None else None, _stream()))

    def tracers_primitive_variables(self) -> torch.Tensor:
        """rdyhip_tracers_primitive_variables: [owned, 3 + NT] (h, u, v, c_0 ...) as a view of the device array; stored by every
        tracer evaluation after the first request, zeros until one has run"""
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(_lib.load().rdyhip_tracers_primitive_variables(self._h, C.byref(p), C.byref(n)))
        ncomp = 3 + self.num_tracers
        if n.value == 0:
            return torch.zeros((0, ncomp), dtype=torch.float64, device="cuda")
        return torch.as_tensor(_DeviceArray(p.value, (n.value,), self), device="cuda").view(-1, ncomp)

    def tracers_boundary_fluxes(self, boundary: int) -> np.ndarray:
        """rdyhip_tracers_get_boundary_fluxes: [num_edges, 3 + NT] fluxes through the edges of `boundary` (rows of edges whose
        left cell is a ghost are not written)"""
        n = self.mesh.boundaries[boundary].num_edges if 0 <= boundary < len(self.mesh.boundaries) else 0
        out = np.zeros((n, 3 + self.num_tracers))
        _lib.check(_lib.load().rdyhip_tracers_get_boundary_fluxes(self._h, int(boundary), n, out.ctypes.data_as(_lib.c_double_p) if out.size else None))
        return out

    # -- tracer output (rdyhip_tracer_state_* / _error_sums / _output_mean_* / _series_*): the read-out, error sums, output means
    # and observation series of the [num_cells, 3 + NT] state; `comps`: bit i = component i of the row --------------------------
    def _tracer_mask_bits(self, comps: int) -> int:
        n = 3 + self.num_tracers
        return bin(int(comps)).count("1") if 1 <= int(comps) < (1 << n) else 0

    def tracers_state_planes(self, u_local: torch.Tensor, comps: int, form: int = TRACER_FORM_CONSERVED,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """rdyhip_tracer_state_planes: [popcount(comps), owned] device tensor, plane k = the k-th component in `comps`
        (ascending) of the owned cells' rows -- TRACER_FORM_CONSERVED: bit for bit; TRACER_FORM_PRIMITIVE: (h, u, v, c_0 ...) as a
        tracer evaluation stores them; one launch on the current stream.  `out`: as Operator.state_planes."""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        k, no = self._tracer_mask_bits(comps), self.mesh.num_owned_cells
        if out is None:
            out = torch.empty((k, no), dtype=torch.float64, device="cuda")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= k * no):
            raise RDyHipError(83, f"out must be a contiguous float64 device tensor of at least {k} x {no} values")
        _lib.check(_lib.load().rdyhip_tracer_state_planes(self._h, int(comps), int(form), _ptr(u_local), _ptr(out), _stream()))
        return out

    def tracers_read_state_begin(self, u_local: torch.Tensor, comps: int, form: int = TRACER_FORM_CONSERVED):
        """rdyhip_tracer_state_read_begin: as read_state_begin, for the tracer state, with buffers of its own"""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        _lib.check(_lib.load().rdyhip_tracer_state_read_begin(self._h, int(comps), int(form), _ptr(u_local), _stream()))

    def tracers_read_state_ready(self) -> bool:
        """rdyhip_tracer_state_read_ready: the copy of the last tracers_read_state_begin has finished (an event query)"""
        out = C.c_int32()
        _lib.check(_lib.load().rdyhip_tracer_state_read_ready(self._h, C.byref(out)))
        return bool(out.value)

    def tracers_read_state(self, comp: int) -> np.ndarray:
        """rdyhip_tracer_state_read_wait + _get: waits for the copy of the last tracers_read_state_begin (for that alone) and
        returns component `comp` (exactly one bit) of the owned cells as a numpy array"""
        lib = _lib.load()
        _lib.check(lib.rdyhip_tracer_state_read_wait(self._h))
        out = np.empty(self.mesh.num_owned_cells)
        _lib.check(lib.rdyhip_tracer_state_read_get(self._h, int(comp), int(out.size), out.ctypes.data_as(_lib.c_double_p) if out.size else None))
        return out

    def tracers_error_sums(self, u_local: torch.Tensor, exact: Optional[torch.Tensor] = None) -> dict:
        """rdyhip_tracer_error_sums + _get: {"l1", "l2_squared", "linf": [3 + NT] arrays, "area": float} of u_local - exact over
        the owned cells of this rank (`exact`: [owned, 3 + NT] device tensor; None: zeros); the flow columns are the bits of
        error_sums for the [cell, 3] slice.  The reduction over ranks and the square root are the caller's."""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        self._check_tracer_state(exact, "exact", self.mesh.num_owned_cells, optional=True)
        lib = _lib.load()
        _lib.check(lib.rdyhip_tracer_error_sums(self._h, _ptr(u_local), _ptr(exact) if exact is not None else None, _stream()))
        s = _lib.RDyHipTracerErrorSums()
        _lib.check(lib.rdyhip_tracer_error_sums_get(self._h, C.byref(s)))
        n = 3 + self.num_tracers
        return {"l1": np.array(s.l1[:n]), "l2_squared": np.array(s.l2_squared[:n]), "linf": np.array(s.linf[:n]), "area": float(s.area),
                "padding": np.array(s.l1[n:] + s.l2_squared[n:] + s.linf[n:])}

    def tracers_enable_output_means(self, vars: int):
        """rdyhip_tracer_output_mean_enable: a zeroed [owned, 3 + NT] accumulator for each of OUTPUT_* in `vars` that has none yet"""
        _lib.check(_lib.load().rdyhip_tracer_output_mean_enable(self._h, int(vars)))

    def tracers_accumulate_output_means(self, vars: int, dt: float, u_solution: Optional[torch.Tensor] = None,
                                        u_primitive: Optional[torch.Tensor] = None):
        """rdyhip_tracer_output_mean_accumulate: all of `vars` in one launch on the current stream -- the solution from
        `u_solution`, the primitive variables formed from `u_primitive` (the state the evaluation saw: after a fused Euler step
        its input), the sources from the operator's arrays; each state [num_cells, 3 + NT], needed only with its variable"""
        self._check_tracer_state(u_solution, "u_solution", self.mesh.num_cells, optional=True)
        self._check_tracer_state(u_primitive, "u_primitive", self.mesh.num_cells, optional=True)
        _lib.check(_lib.load().rdyhip_tracer_output_mean_accumulate(self._h, int(vars), float(dt), _ptr(u_solution) if u_solution is not None else None,
                                                                   _ptr(u_primitive) if u_primitive is not None else None, _stream()))

    def tracers_output_mean(self, var: int):
        """rdyhip_tracer_output_mean_get: (mean [owned, 3 + NT], accumulated time) of one variable; nothing is reset"""
        out = torch.empty((self.mesh.num_owned_cells, 3 + self.num_tracers), dtype=torch.float64, device="cuda")
        t = C.c_double()
        _lib.check(_lib.load().rdyhip_tracer_output_mean_get(self._h, int(var), _ptr(out), C.byref(t), _stream()))
        return out, t.value

    def tracers_reset_output_means(self, vars: int):
        """rdyhip_tracer_output_mean_reset: accumulators and times of `vars` back to zero, on the current stream"""
        _lib.check(_lib.load().rdyhip_tracer_output_mean_reset(self._h, int(vars), _stream()))

    def tracers_output_mean_time(self, var: int) -> float:
        t = C.c_double()
        _lib.check(_lib.load().rdyhip_tracer_output_mean_time(self._h, int(var), C.byref(t)))
        return t.value

    def tracers_enable_observation_series(self, owned_cell_ids, capacity: int):
        """rdyhip_tracer_series_enable: a device log of `capacity` records of the 3 + NT-wide state in the cells `owned_cell_ids`
        (owned-cell indices; a site may repeat)"""
        ids = np.ascontiguousarray(owned_cell_ids, dtype=np.int32).ravel()
        arg = ids if ids.size else np.zeros(1, dtype=np.int32)
        _lib.check(_lib.load().rdyhip_tracer_series_enable(self._h, int(ids.size), arg.ctypes.data_as(_lib.c_int32_p), int(capacity)))

    def tracers_series_record(self, time: float, u_local: torch.Tensor):
        """rdyhip_tracer_series_record: one record of the state `u_local` appended to the log, one launch on the current stream"""
        self._check_tracer_state(u_local, "u_local", self.mesh.num_cells)
        _lib.check(_lib.load().rdyhip_tracer_series_record(self._h, float(time), _ptr(u_local), _stream()))

    def tracers_series_info(self) -> dict:
        """rdyhip_tracer_series_info: rows of a record, records in the log, capacity"""
        e, n, cap = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.load().rdyhip_tracer_series_info(self._h, C.byref(e), C.byref(n), C.byref(cap)))
        return {"entries": e.value, "count": n.value, "capacity": cap.value}

    def tracers_series_read(self, first: int = 0, count: Optional[int] = None):
        """rdyhip_tracer_series_read: (times [count], values [count, entries, 3 + NT]) of records [first, first + count) as numpy
        arrays (count=None: all from `first`); synchronises the current stream"""
        info = self.tracers_series_info()
        if count is None:
            count = max(info["count"] - int(first), 0)
        times = np.zeros(max(int(count), 0))
        values = np.zeros((max(int(count), 0), info["entries"], 3 + self.num_tracers))
        tp = times.ctypes.data_as(_lib.c_double_p) if times.size else None
        vp = values.ctypes.data_as(_lib.c_double_p) if values.size else None
        _lib.check(_lib.load().rdyhip_tracer_series_read(self._h, int(first), int(count), tp, vp, _stream()))
        return times, values

    def tracers_series_clear(self):
        """rdyhip_tracer_series_clear: the log holds no records"""
        _lib.check(_lib.load().rdyhip_tracer_series_clear(self._h))

    # -- ensembles (src/ensemble.c): B members on this mesh, state [B, num_cells, 3], one launch per evaluation ---------------------
    num_members = 0

    def enable_ensemble(self, num_members: int, well_balancing: int = WELL_BALANCING_NONE):
        """rdyhip_ensemble_enable: `num_members` (1..64) members, each starting with the operator's current Manning's n, external
        source and boundary values; a member then overrides only what differs.  well_balancing=WELL_BALANCING_HR:
        rdyhip_ens_hr_enable, the same on an operator created with hydrostatic reconstruction (every ensemble call then runs
        ensemble_hr_kernel)"""
        if well_balancing == WELL_BALANCING_HR:
            _lib.check(_lib.load().rdyhip_ens_hr_enable(self._h, int(num_members)))
        elif well_balancing == WELL_BALANCING_NONE:
            _lib.check(_lib.load().rdyhip_ensemble_enable(self._h, int(num_members)))
        else:
            raise ValueError(f"well_balancing is WELL_BALANCING_NONE or WELL_BALANCING_HR, not {well_balancing}")
        self.num_members = int(num_members)

    def ensemble_well_balancing(self) -> int:
        """rdyhip_ens_hr_info: WELL_BALANCING_HR after enable_ensemble(..., well_balancing=WELL_BALANCING_HR), else WELL_BALANCING_NONE"""
        wb = C.c_int32()
        _lib.check(_lib.load().rdyhip_ens_hr_info(self._h, C.byref(wb)))
        return wb.value

    def ensemble_info(self) -> int:
        """rdyhip_ensemble_info: the number of members, 0: not enabled"""
        n = C.c_int32()
        _lib.check(_lib.load().rdyhip_ensemble_info(self._h, C.byref(n)))
        return n.value

    def _check_ensemble_state(self, t, name: str, cells: int, optional: bool = False):
        if optional and t is None:
            return
        b = self.num_members
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == 3 * b * cells):
            raise RDyHipError(83, f"{name} must be a contiguous float64 device tensor of {b} members x {cells} cells x 3")

    def _ensemble_dts(self, dts):
        d = np.ascontiguousarray(dts, dtype=np.float64).ravel()
        if d.size != self.num_members:
            raise RDyHipError(83, f"dts must hold one dt per member ({self.num_members}), not {d.size}")
        return d

    @staticmethod
    def _region(values, owned_cell_ids):
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        ip, ids = None, None
        if owned_cell_ids is not None:
            ids = np.ascontiguousarray(owned_cell_ids, dtype=np.int32).ravel()
            if ids.size != v.size:
                raise RDyHipError(60, f"size ({v.size}) does not match the region size ({ids.size})")
            ip = ids.ctypes.data_as(_lib.c_int32_p)
        return v, ids, ip

    def ensemble_set_mannings_n(self, member: int, values, owned_cell_ids=None):
        """rdyhip_ensemble_set_mannings: member `member`'s Manning's n in the owned cells `owned_cell_ids` (None: cells 0 .. n - 1)"""
        v, ids, ip = self._region(values, owned_cell_ids)
        _lib.check(_lib.load().rdyhip_ensemble_set_mannings(self._h, int(member), int(v.size), ip, v.ctypes.data_as(_lib.c_double_p) if v.size else None))

    def ensemble_set_external_source(self, member: int, comp: int, values, owned_cell_ids=None):
        """rdyhip_ensemble_set_external_source: component `comp` of member `member`'s source"""
        v, ids, ip = self._region(values, owned_cell_ids)
        _lib.check(_lib.load().rdyhip_ensemble_set_external_source(self._h, int(member), int(comp), int(v.size), ip,
                                                                   v.ctypes.data_as(_lib.c_double_p) if v.size else None))

    def ensemble_set_boundary_values(self, member: int, boundary: int, values):
        """values[e, :] = (h, hu, hv) of boundary edge e for member `member` (rdyhip_ensemble_set_boundary_values)"""
        v = np.ascontiguousarray(values, dtype=np.float64)
        ne = v.shape[0] if v.ndim == 2 and v.shape[1] == 3 else -1
        _lib.check(_lib.load().rdyhip_ensemble_set_boundary_values(self._h, int(member), int(boundary), int(ne),
                                                                   v.ctypes.data_as(_lib.c_double_p) if v.size else None))

    def ensemble_rhs_function(self, dts, u_local: torch.Tensor, f_global: torch.Tensor):
        """rdyhip_ensemble_rhs_function: f_global [B, owned, 3] = F_m(u_local [B, num_cells, 3]) with dts[m], every member's
        diagnostics reset, one launch"""
        d = self._ensemble_dts(dts)
        self._check_ensemble_state(u_local, "u_local", self.mesh.num_cells)
        self._check_ensemble_state(f_global, "f_global", self.mesh.num_owned_cells)
        _lib.check(_lib.load().rdyhip_ensemble_rhs_function(self._h, d.ctypes.data_as(_lib.c_double_p), _ptr(u_local), _ptr(f_global), _stream()))

    def ensemble_euler_step(self, dts, u_local: torch.Tensor, u_out: torch.Tensor, f_global: Optional[torch.Tensor] = None):
        """rdyhip_ensemble_euler_step: u_out[m, owned rows] = fma(dts[m], F_m, u_local), not in place; f_global=None: F is never stored"""
        d = self._ensemble_dts(dts)
        self._check_ensemble_state(u_local, "u_local", self.mesh.num_cells)
        self._check_ensemble_state(u_out, "u_out", self.mesh.num_cells)
        self._check_ensemble_state(f_global, "f_global", self.mesh.num_owned_cells, optional=True)
        _lib.check(_lib.load().rdyhip_ensemble_euler_step(self._h, d.ctypes.data_as(_lib.c_double_p), _ptr(u_local), _ptr(u_out),
                                                          _ptr(f_global) if f_global is not None else None, _stream()))

    def ensemble_boundary_fluxes(self, member: int, boundary: int) -> np.ndarray:
        """rdyhip_ensemble_get_boundary_fluxes: [num_edges, 3] fluxes of member `member` through the edges of `boundary` (rows of
        edges whose left cell is a ghost are not written)"""
        n = self.mesh.boundaries[boundary].num_edges if 0 <= boundary < len(self.mesh.boundaries) else 0
        out = np.zeros((n, 3))
        _lib.check(_lib.load().rdyhip_ensemble_get_boundary_fluxes(self._h, int(member), int(boundary), n,
                                                                   out.ctypes.data_as(_lib.c_double_p) if out.size else None))
        return out

    def ensemble_update_diagnostics(self):
        _lib.check(_lib.load().rdyhip_ensemble_update_diagnostics(self._h, _stream()))

    def ensemble_diagnostics_begin(self):
        """the non-blocking half of ensemble_update_diagnostics (rdyhip_diagnostics_begin, ensemble scope), on the current stream"""
        _lib.check(_lib.load().rdyhip_diagnostics_begin(self._h, DIAGNOSTICS_ENSEMBLE, _stream()))

    def ensemble_diagnostics_wait(self):
        _lib.check(_lib.load().rdyhip_diagnostics_wait(self._h, DIAGNOSTICS_ENSEMBLE))

    def ensemble_get_diagnostics(self) -> list:
        """rdyhip_ensemble_get_diagnostics: one CourantNumberDiagnostics per member"""
        c = (_lib.RDyHipCourant * max(self.num_members, 1))()
        _lib.check(_lib.load().rdyhip_ensemble_get_diagnostics(self._h, c))
        return [CourantNumberDiagnostics(c[m].max_courant_num, c[m].global_edge_id, c[m].global_cell_id) for m in range(self.num_members)]

    # -- ensemble output (rdyhip_ens_state_* / _error_sums / _output_mean_* / _series_* / _stats): the read-out, error sums, output
    # means, observation series and member statistics of the [B, num_cells, 3] state, every call one launch for all members -------
    @staticmethod
    def _mask_bits(comps: int) -> int:
        return bin(int(comps)).count("1") if 1 <= int(comps) <= 7 else 0

    def _ensemble_per_member(self, values, name: str):
        d = np.ascontiguousarray(values, dtype=np.float64).ravel()
        if d.size != self.num_members:
            raise RDyHipError(83, f"{name} must hold one value per member ({self.num_members}), not {d.size}")
        return d

    def ensemble_state_planes(self, u_local: torch.Tensor, comps: int) -> torch.Tensor:
        """rdyhip_ens_state_planes: [B, popcount(comps), owned] device tensor, plane [m, k] = the k-th component of `comps`
        (ascending) of member m's owned cells, bit for bit; one launch on the current stream"""
        self._check_ensemble_state(u_local, "u_local", self.mesh.num_cells)
        out = torch.empty((self.num_members, self._mask_bits(comps), self.mesh.num_owned_cells), dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().rdyhip_ens_state_planes(self._h, int(comps), _ptr(u_local), _ptr(out), _stream()))
        return out

    def ensemble_read_state_begin(self, u_local: torch.Tensor, comps: int):
        """rdyhip_ens_state_read_begin: as read_state_begin, for all members in one launch and one copy, with buffers of its own"""
        self._check_ensemble_state(u_local, "u_local", self.mesh.num_cells)
        _lib.check(_lib.load().rdyhip_ens_state_read_begin(self._h, int(comps), _ptr(u_local), _stream()))

    def ensemble_read_state_ready(self) -> bool:
        """rdyhip_ens_state_read_ready: the copy of the last ensemble_read_state_begin has finished (an event query)"""
        out = C.c_int32()
        _lib.check(_lib.load().rdyhip_ens_state_read_ready(self._h, C.byref(out)))
        return bool(out.value)

    def ensemble_read_state(self, member: int, comp: int) -> np.ndarray:
        """rdyhip_ens_state_read_wait + _get: waits for the copy of the last ensemble_read_state_begin (for that alone) and returns
        component `comp` (exactly one COMPONENT_*) of member `member`'s owned cells as a numpy array"""
        lib = _lib.load()
        _lib.check(lib.rdyhip_ens_state_read_wait(self._h))
        out = np.empty(self.mesh.num_owned_cells)
        _lib.check(lib.rdyhip_ens_state_read_get(self._h, int(member), int(comp), int(out.size),
                                                 out.ctypes.data_as(_lib.c_double_p) if out.size else None))
        return out

    def ensemble_error_sums(self, u_local: torch.Tensor, exact: Optional[torch.Tensor] = None) -> list:
        """rdyhip_ens_error_sums + _get: one dict of Operator.error_sums per member, of u_local[m] - exact[m] over the owned cells
        (`exact`: [B, owned, 3] device tensor; None: zeros); two launches for all members; member m's dict holds the bits
        error_sums gives for member m's slice"""
        self._check_ensemble_state(u_local, "u_local", self.mesh.num_cells)
        self._check_ensemble_state(exact, "exact", self.mesh.num_owned_cells, optional=True)
        lib = _lib.load()
        _lib.check(lib.rdyhip_ens_error_sums(self._h, _ptr(u_local), _ptr(exact) if exact is not None else None, _stream()))
        s = (_lib.RDyHipErrorSums * max(self.num_members, 1))()
        _lib.check(lib.rdyhip_ens_error_sums_get(self._h, s))
        return [{"l1": np.array(s[m].l1[:]), "l2_squared": np.array(s[m].l2_squared[:]), "linf": np.array(s[m].linf[:]), "area": float(s[m].area)}
                for m in range(self.num_members)]

    def ensemble_enable_output_means(self, vars: int):
        """rdyhip_ens_output_mean_enable: a zeroed [B, owned, 3] accumulator for each of OUTPUT_* in `vars` that has none yet"""
        _lib.check(_lib.load().rdyhip_ens_output_mean_enable(self._h, int(vars)))

    def ensemble_accumulate_output_means(self, vars: int, dts, u_solution: Optional[torch.Tensor] = None,
                                         u_primitive: Optional[torch.Tensor] = None):
        """rdyhip_ens_output_mean_accumulate: all of `vars` of all members in one launch on the current stream, member m weighted
        with dts[m] -- the solution from `u_solution`, the primitive variables formed from `u_primitive` (the state the evaluation
        saw: after a fused Euler step its input), the sources from the members' own; each state [B, num_cells, 3], needed only
        with its variable"""
        d = self._ensemble_per_member(dts, "dts")
        self._check_ensemble_state(u_solution, "u_solution", self.mesh.num_cells, optional=True)
        self._check_ensemble_state(u_primitive, "u_primitive", self.mesh.num_cells, optional=True)
        _lib.check(_lib.load().rdyhip_ens_output_mean_accumulate(self._h, int(vars), d.ctypes.data_as(_lib.c_double_p),
                                                                _ptr(u_solution) if u_solution is not None else None,
                                                                _ptr(u_primitive) if u_primitive is not None else None, _stream()))

    def ensemble_output_mean(self, var: int):
        """rdyhip_ens_output_mean_get: (means [B, owned, 3], accumulated times [B]) of one variable; nothing is reset"""
        out = torch.empty((self.num_members, self.mesh.num_owned_cells, 3), dtype=torch.float64, device="cuda")
        t = np.zeros(max(self.num_members, 1))
        _lib.check(_lib.load().rdyhip_ens_output_mean_get(self._h, int(var), _ptr(out), t.ctypes.data_as(_lib.c_double_p), _stream()))
        return out, t[:self.num_members]

    def ensemble_reset_output_means(self, vars: int):
        """rdyhip_ens_output_mean_reset: accumulators and every member's time of `vars` back to zero, on the current stream"""
        _lib.check(_lib.load().rdyhip_ens_output_mean_reset(self._h, int(vars), _stream()))

    def ensemble_output_mean_time(self, var: int) -> np.ndarray:
        """rdyhip_ens_output_mean_time: [B] the time every member has accumulated for `var`"""
        t = np.zeros(max(self.num_members, 1))
        _lib.check(_lib.load().rdyhip_ens_output_mean_time(self._h, int(var), t.ctypes.data_as(_lib.c_double_p)))
        return t[:self.num_members]

    def ensemble_enable_observation_series(self, owned_cell_ids, capacity: int):
        """rdyhip_ens_series_enable: a device log of `capacity` records of every member's state in the cells `owned_cell_ids`
        (owned-cell indices; a site may repeat)"""
        ids = np.ascontiguousarray(owned_cell_ids, dtype=np.int32).ravel()
        arg = ids if ids.size else np.zeros(1, dtype=np.int32)
        _lib.check(_lib.load().rdyhip_ens_series_enable(self._h, int(ids.size), arg.ctypes.data_as(_lib.c_int32_p), int(capacity)))

    def ensemble_series_record(self, times, u_local: torch.Tensor):
        """rdyhip_ens_series_record: one record [B, sites, 3] of the state `u_local` appended to the log at the members' `times`
        ([B]), one launch on the current stream"""
        t = self._ensemble_per_member(times, "times")
        self._check_ensemble_state(u_local, "u_local", self.mesh.num_cells)
        _lib.check(_lib.load().rdyhip_ens_series_record(self._h, t.ctypes.data_as(_lib.c_double_p), _ptr(u_local), _stream()))

    def ensemble_series_info(self) -> dict:
        """rdyhip_ens_series_info: sites of a record, records in the log, capacity"""
        e, n, cap = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.load().rdyhip_ens_series_info(self._h, C.byref(e), C.byref(n), C.byref(cap)))
        return {"entries": e.value, "count": n.value, "capacity": cap.value}

    def ensemble_series_read(self, first: int = 0, count: Optional[int] = None):
        """rdyhip_ens_series_read: (times [count, B], values [count, B, sites, 3]) of records [first, first + count) as numpy arrays
        (count=None: all from `first`); synchronises the current stream"""
        info = self.ensemble_series_info()
        if count is None:
            count = max(info["count"] - int(first), 0)
        times = np.zeros((max(int(count), 0), self.num_members))
        values = np.zeros((max(int(count), 0), self.num_members, info["entries"], 3))
        tp = times.ctypes.data_as(_lib.c_double_p) if times.size else None
        vp = values.ctypes.data_as(_lib.c_double_p) if values.size else None
        _lib.check(_lib.load().rdyhip_ens_series_read(self._h, int(first), int(count), tp, vp, _stream()))
        return times, values

    def ensemble_series_clear(self):
        """rdyhip_ens_series_clear: the log holds no records"""
        _lib.check(_lib.load().rdyhip_ens_series_clear(self._h))

    def ensemble_stats(self, u_local: torch.Tensor, comps: int) -> torch.Tensor:
        """rdyhip_ens_stats: [popcount(comps), 3, owned] device tensor, planes [k, 0..2] = mean, minimum and maximum over the members
        of the k-th component of `comps` in every owned cell; one launch on the current stream.  The mean adds the members in
        order and multiplies by 1 / B once; minimum and maximum are comparisons in member order: of equal values (+0.0 and -0.0
        too) the earlier member's bits stay, a NaN in a later member is passed over, a NaN in member 0 stays."""
        self._check_ensemble_state(u_local, "u_local", self.mesh.num_cells)
        out = torch.empty((self._mask_bits(comps), 3, self.mesh.num_owned_cells), dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().rdyhip_ens_stats(self._h, int(comps), _ptr(u_local), _ptr(out), _stream()))
        return out

    # -- second order: ComputeLeastSquaresGradients for the owned cells (src/operator_fluxes_ceed.c:998-1042)
    def compute_gradients(self, u_local: torch.Tensor, phase: int = PHASE_ALL):
        _lib.check(_lib.load().rdyhip_compute_gradients(self._h, int(phase), _ptr(u_local), _stream()))

    @property
    def gradients(self) -> torch.Tensor:
        """[num_cells, 6] (dh/dx, dh/dy, dhu/dx, dhu/dy, dhv/dx, dhv/dy) by LOCAL cell; ghost rows are the caller's to fill"""
        return self._field(4, 6)

    # -- SetOperatorBoundaryValues (src/operator.c:1045-1061) --------------
    def set_boundary_values(self, boundary: int, values, comp_offset: int = 0, ordered: bool = False):
        """values[e, c] for component comp_offset+c of boundary edge e (RDySetFlowDirichletBoundaryValues,
        src/rdydata.c:88-106).  `ordered`: the stream-ordered form (rdyhip_set_boundary_values_on, current stream) -- no
        device synchronisation, no blocking copy; the default synchronises as the legacy entry point does."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim == 1:
            v = v.reshape(-1, 1)
        if ordered:
            _lib.check(_lib.load().rdyhip_set_boundary_values_on(self._h, int(boundary), int(comp_offset), int(v.shape[1]),
                                                                int(v.shape[0]), v.ctypes.data_as(_lib.c_double_p), _stream()))
            return
        _lib.check(_lib.load().rdyhip_set_boundary_values(self._h, int(boundary), int(comp_offset), int(v.shape[1]),
                                                         int(v.shape[0]), v.ctypes.data_as(_lib.c_double_p)))

    # -- ExtractOperatorBoundaryFluxes ----------------------------------------
    def boundary_fluxes(self, boundary: int, accumulated: bool = False) -> np.ndarray:
        n = self.mesh.boundaries[boundary].num_edges
        out = np.zeros((n, 3))
        _lib.check(_lib.load().rdyhip_get_boundary_fluxes(self._h, int(boundary), 1 if accumulated else 0, n,
                                                         out.ctypes.data_as(_lib.c_double_p)))
        return out

    def reset_boundary_fluxes_accum(self):
        _lib.check(_lib.load().rdyhip_reset_boundary_fluxes_accum(self._h))

    # -- external sources (RDySet{Regional,Domain}{Water,XMomentum,YMomentum}Source, src/rdydata.c:225-366)
    def set_domain_external_source(self, comp: int, values, ordered: bool = False):
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        if v.size != self.mesh.num_owned_cells:
            raise RDyHipError(60, f"size ({v.size}) does not match the number of owned cells ({self.mesh.num_owned_cells})")
        if ordered:
            _lib.check(_lib.load().rdyhip_set_external_source_on(self._h, int(comp), int(v.size), None, v.ctypes.data_as(_lib.c_double_p), _stream()))
            return
        _lib.check(_lib.load().rdyhip_set_external_source(self._h, int(comp), int(v.size), None, v.ctypes.data_as(_lib.c_double_p)))

    def set_regional_external_source(self, owned_cell_ids, comp: int, values, ordered: bool = False):
        ids = np.ascontiguousarray(owned_cell_ids, dtype=np.int32).ravel()
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        if v.size != ids.size:
            raise RDyHipError(60, f"size ({v.size}) does not match the region size ({ids.size})")
        if ordered:
            _lib.check(_lib.load().rdyhip_set_external_source_on(self._h, int(comp), int(v.size), ids.ctypes.data_as(_lib.c_int32_p),
                                                                v.ctypes.data_as(_lib.c_double_p), _stream()))
            return
        _lib.check(_lib.load().rdyhip_set_external_source(self._h, int(comp), int(v.size), ids.ctypes.data_as(_lib.c_int32_p),
                                                         v.ctypes.data_as(_lib.c_double_p)))

    # -- Manning's n (RDySet{Regional,Domain}ManningsN, src/rdydata.c:506-539)
    def set_domain_mannings_n(self, values, ordered: bool = False):
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        if v.size != self.mesh.num_owned_cells:
            raise RDyHipError(60, f"size ({v.size}) does not match the number of owned cells ({self.mesh.num_owned_cells})")
        if ordered:
            _lib.check(_lib.load().rdyhip_set_mannings_on(self._h, int(v.size), None, v.ctypes.data_as(_lib.c_double_p), _stream()))
            return
        _lib.check(_lib.load().rdyhip_set_mannings(self._h, int(v.size), None, v.ctypes.data_as(_lib.c_double_p)))

    def set_regional_mannings_n(self, owned_cell_ids, values, ordered: bool = False):
        ids = np.ascontiguousarray(owned_cell_ids, dtype=np.int32).ravel()
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        if v.size != ids.size:
            raise RDyHipError(60, f"size ({v.size}) does not match the region size ({ids.size})")
        if ordered:
            _lib.check(_lib.load().rdyhip_set_mannings_on(self._h, int(v.size), ids.ctypes.data_as(_lib.c_int32_p),
                                                         v.ctypes.data_as(_lib.c_double_p), _stream()))
            return
        _lib.check(_lib.load().rdyhip_set_mannings(self._h, int(v.size), ids.ctypes.data_as(_lib.c_int32_p),
                                                  v.ctypes.data_as(_lib.c_double_p)))

    def refresh_field(self, field: int, values):
        """rdyhip_refresh_field: a whole input field (1: external sources [owned,3]; 2: Manning n [owned]) from a host array or a
        device tensor, ordered on the current stream"""
        if isinstance(values, torch.Tensor) and values.is_cuda:
            t = values.contiguous()
            _lib.check(_lib.load().rdyhip_refresh_field(self._h, int(field), _ptr(t), int(t.numel()), 1, _stream()))
            return
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        _lib.check(_lib.load().rdyhip_refresh_field(self._h, int(field), v.ctypes.data, int(v.size), 0, _stream()))

    # -- device-resident fields ------------------------------------------------
    def _field(self, field: int, ncomp: int) -> torch.Tensor:
        p = C.c_void_p()
        n = C.c_int64()
        _lib.check(_lib.load().rdyhip_field_ptr(self._h, int(field), C.byref(p), C.byref(n)))
        if n.value == 0:
            return torch.zeros((0, ncomp), dtype=torch.float64, device="cuda")
        t = torch.as_tensor(_DeviceArray(p.value, (n.value,), self), device="cuda")
        return t.view(-1, ncomp) if ncomp > 1 else t

    @property
    def primitive_variables(self) -> torch.Tensor:
        """Operator.primitive_variables: [owned,3] (h,u,v).  Written by every evaluation from the first time it is asked for
        (until release_primitive_variables); asked for after evaluations that did not store them, it is first filled from the
        u_local of the most recent one, which must still hold that state (rdyhip_field_ptr in include/rdyhip.h; the operator
        keeps that tensor alive, writing it in place before asking is the caller's business)."""
        return self._field(0, 3)

    def release_primitive_variables(self):
        """rdyhip_field_release: tensors obtained from `primitive_variables` are not read until it is asked for again;
        evaluations stop storing them."""
        _lib.check(_lib.load().rdyhip_field_release(self._h, 0))

    def primitive_variables_stored(self) -> bool:
        """rdyhip_primitive_variables_stored: evaluations store the primitive variables (somebody has asked for them)."""
        out = C.c_int32()
        _lib.check(_lib.load().rdyhip_primitive_variables_stored(self._h, C.byref(out)))
        return bool(out.value)

    @property
    def external_sources(self) -> torch.Tensor:
        return self._field(1, 3)

    def source_is_water_only(self) -> bool:
        """rdyhip_source_is_water_only: the first-order / HR kernels read the water source from its own [owned] plane (every
        momentum source is known to be +0.0).  Reading `external_sources` hands out a writable pointer and ends that for good."""
        out = C.c_int32()
        _lib.check(_lib.load().rdyhip_source_is_water_only(self._h, C.byref(out)))
        return bool(out.value)

    def uniform_fields(self) -> int:
        """rdyhip_uniform_fields: the UNIFORM_* bits of the fields whose every owned element is known to hold one value -- the
        next first-order / HR launch reads element 0 of them instead of the plane (include/rdyhip.h, "Uniform fields").  Reading
        `external_sources` or `mannings_n` hands out a writable pointer and ends that field's mode for good."""
        out = C.c_int32()
        _lib.check(_lib.load().rdyhip_uniform_fields(self._h, C.byref(out)))
        return int(out.value)

    def normal_table_info(self) -> Tuple[int, bool]:
        """rdyhip_normal_table_info: (entries, active) -- active: the operator's first-order / HR launches take the edge normals
        from its table of `entries` distinct ones (kernel family swe_rhs_ntab_kernel); (0, False): they stream them."""
        n, act = C.c_int32(), C.c_int32()
        _lib.check(_lib.load().rdyhip_normal_table_info(self._h, C.byref(n), C.byref(act)))
        return int(n.value), bool(act.value)

    @property
    def mannings_n(self) -> torch.Tensor:
        return self._field(2, 1)

    def enable_flux_divergence(self, enable: bool = True):
        _lib.check(_lib.load().rdyhip_enable_flux_divergence(self._h, 1 if enable else 0))

    @property
    def flux_divergence(self) -> torch.Tensor:
        return self._field(3, 3)

    # -- diagnostics (src/operator.c:772-784, 867-893) ---------------------
    def reset_diagnostics(self):
        _lib.check(_lib.load().rdyhip_reset_diagnostics(self._h, _stream()))

    def update_diagnostics(self):
        _lib.check(_lib.load().rdyhip_update_diagnostics(self._h, _stream()))

    def get_diagnostics(self) -> CourantNumberDiagnostics:
        c = _lib.RDyHipCourant()
        _lib.check(_lib.load().rdyhip_get_diagnostics(self._h, C.byref(c)))
        return CourantNumberDiagnostics(c.max_courant_num, c.global_edge_id, c.global_cell_id)

    # the same read-back in two halves (rdyhip_diagnostics_*): begin enqueues the merge launch, a 16-byte copy into pinned
    # memory and an event on the current stream and returns; wait blocks on that event alone and stores what get_diagnostics
    # returns.  The result is that of begin's place in the stream.
    def diagnostics_begin(self):
        _lib.check(_lib.load().rdyhip_diagnostics_begin(self._h, DIAGNOSTICS_OPERATOR, _stream()))

    def diagnostics_ready(self) -> bool:
        """an event query; it never stands in for diagnostics_wait"""
        r = C.c_int32(0)
        _lib.check(_lib.load().rdyhip_diagnostics_ready(self._h, DIAGNOSTICS_OPERATOR, C.byref(r)))
        return bool(r.value)

    def diagnostics_wait(self):
        _lib.check(_lib.load().rdyhip_diagnostics_wait(self._h, DIAGNOSTICS_OPERATOR))

    # -- explicit Euler update kept on the device ----------------------------
    def axpy_owned(self, dt: float, f_global: torch.Tensor, u_local: torch.Tensor):
        self._check_vecs(u_local, f_global)
        _lib.check(_lib.load().rdyhip_axpy_owned(self._h, float(dt), _ptr(f_global), _ptr(u_local), _stream()))

    def copy_owned_rows(self, u_global: torch.Tensor, u_local: torch.Tensor):
        """the local half of DMGlobalToLocal (src/rdysetup.c:1133-1134): u_local[owned cell o] = u_global[o]"""
        self._check_vecs(u_local, u_global)
        _lib.check(_lib.load().rdyhip_copy_owned_rows(self._h, _ptr(u_global), _ptr(u_local), _stream()))

    def layout_info(self) -> dict:
        info = _lib.RDyHipLayoutInfo()
        _lib.check(_lib.load().rdyhip_layout_info(self._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}


def pack_rows(src: torch.Tensor, row_ids: torch.Tensor, buf: torch.Tensor):
    """buf[i, :] = src[row_ids[i], :] for a [rows, ncomp] device array (the gradient field)"""
    _lib.check(_lib.load().rdyhip_pack_rows(_ptr(src), int(src.shape[1]), _ptr(row_ids), int(row_ids.numel()), _ptr(buf), _stream()))


def unpack_rows(dst: torch.Tensor, row_ids: torch.Tensor, buf: torch.Tensor):
    _lib.check(_lib.load().rdyhip_unpack_rows(_ptr(dst), int(dst.shape[1]), _ptr(row_ids), int(row_ids.numel()), _ptr(buf), _stream()))


def pack_cells(u_local: torch.Tensor, cell_ids: torch.Tensor, buf: torch.Tensor):
    """buf[i] = u_local[cell_ids[i]] on the current stream (halo send side)."""
    _lib.check(_lib.load().rdyhip_pack_cells(_ptr(u_local), _ptr(cell_ids), int(cell_ids.numel()), _ptr(buf), _stream()))


def unpack_cells(u_local: torch.Tensor, cell_ids: torch.Tensor, buf: torch.Tensor):
    """u_local[cell_ids[i]] = buf[i] on the current stream (halo receive side)."""
    _lib.check(_lib.load().rdyhip_unpack_cells(_ptr(u_local), _ptr(cell_ids), int(cell_ids.numel()), _ptr(buf), _stream()))
