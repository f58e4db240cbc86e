"""Device-resident explicit time stepping around the RHS operator (SURVEY.md
section 8.f row 1): what PETSc's TSEULER and RDyAdvance do between RHS
evaluations, with the state kept on the GPU.

  * forward Euler: F = RHS(t, U); U += dt F   (TSStep_Euler's VecAXPY; the RHS is
    OperatorRHSFunction, src/rdysetup.c:1120-1172).  `fused=True` (default) does both in
    one pass over the mesh (rdyhip_euler_step: the update rides on the RHS kernel's
    stores, F is never written, two state arrays ping-pong); `fused=False` keeps the
    RHS + axpy pair.
  * classical Runge-Kutta (`temporal="rk4"`: the reference's `numerics.temporal: rk4` = TSRK with TSRK4,
    src/rdysetup.c:1187-1189): four RHS evaluations per step on the stage states U, U + dt/2 k1, U + dt/2 k2, U + dt k3
    -- each one OperatorRHSFunction with its ghost update and the FULL step's dt in the friction term (TSGetTimeStep,
    src/rdysetup.c:1129) -- then U += dt/6 (k1 + 2 k2 + 2 k3 + k4).  Stage vectors stay on the device.  `fused=True`
    (default) takes the whole step in one call behind the C ABI (rdyhip_rk4_step: one launch per stage state, one for the
    final combination) where the operator has it and the halo, if any, is exchanged there too; `fused=False` keeps the
    loop of RHS, copy and axpy calls.  Both give the same bits.
  * time-averaged output (`means`: a mask of the operator's OUTPUT_* bits): what the TS monitor does around TSSolve for
    WriteXDMFOutput's OutputVars (src/xdmf_output.c:436-504) -- one accumulate of dt x (solution, primitive variables,
    sources) for the initial state and one after every step, on the device (rdyhip_output_mean_accumulate).
  * time series (`series`: a TimeSeries): what the TS monitor WriteTimeSeries does (src/time_series.c:530-564) -- the state
    at a list of observation sites every `observation_interval` steps, the accumulated boundary fluxes every
    `boundary_flux_interval` steps -- appended to logs that stay on the device (rdyhip_series_record); nothing is read back
    until the caller asks for the log.
  * RDyAdvance (src/rdyadvance.c:261-383): advance to the next coupling time
    with the last step shortened to land on it (TS_EXACTFINALTIME_MATCHSTEP),
    and, when adaptive time stepping is on, rescale dt from the previous
    interval's maximum Courant number (303-343).  `pipelined=True` takes the read-back of that number in two halves
    (rdyhip_diagnostics_begin / _wait): the forcing of the next interval is applied before the host waits for it.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist


def reduce_courant(diag, device=None, group=None):
    """UpdateOperatorDiagnostics' cross-rank step (src/operator.c:879): the MPI_Allreduce of the
    {max_courant_num, global_edge_id, global_cell_id} struct with FindCourantNumberDiagnostics (705-715), which keeps
    the struct holding the larger value -- so the edge and cell ids of the global maximum travel with it.  One
    all-gather of the three 8-byte words per rank (the value's bit pattern, so nothing is rounded); ties go to the
    lowest rank, a rank without a wet edge contributes (0, -1, -1) as ResetOperatorDiagnostics leaves it (772-784)."""
    from .operator import CourantNumberDiagnostics
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return diag
    import struct
    world = dist.get_world_size(group)
    on_gpu = dist.get_backend(group) == "nccl"
    bits = struct.unpack("<q", struct.pack("<d", float(diag.max_courant_num)))[0]
    mine = torch.tensor([bits, int(diag.global_edge_id), int(diag.global_cell_id)], dtype=torch.int64,
                        device=device if on_gpu else "cpu")
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    rows = torch.stack(parts).cpu().tolist()
    best = CourantNumberDiagnostics(0.0, -1, -1)
    for b, e, c in rows:                      # rank order: a later rank replaces only on a strictly larger value
        v = struct.unpack("<d", struct.pack("<q", b))[0]
        if v > best.max_courant_num:
            best = CourantNumberDiagnostics(v, e, c)
    return best


@dataclasses.dataclass
class AdaptiveTime:
    """RDyTimeAdaptiveSection (include/private/rdyconfigimpl.h): enable,
    target_courant_number, max_increase_factor."""
    target_courant_number: float = 0.5
    max_increase_factor: float = 2.0


@dataclasses.dataclass
class TimeSeries:
    """output.time_series of the reference's configuration (observations.sites / observations.interval, boundary_fluxes) for
    EulerStepper(series=...).  `observation_sites`: owned-cell indices; an interval of 0 turns its series off;
    `boundaries`: the boundaries whose fluxes are recorded (None: all -- the reference leaves out the auto-generated ones);
    `capacity`: records each device log has room for (read the log and clear it before it is full)."""
    observation_sites: Sequence[int] = ()
    observation_interval: int = 0
    boundary_flux_interval: int = 0
    boundaries: Optional[Sequence[int]] = None
    capacity: int = 1024


class EulerStepper:
    """the explicit TS of RDyAdvance: forward Euler (default) or, with temporal="rk4", classical Runge-Kutta"""

    def __init__(self, op, halo=None, adaptive: Optional[AdaptiveTime] = None, fused: bool = True, forcing=None, temporal: str = "euler",
                 means: int = 0, series: Optional[TimeSeries] = None, pipelined: bool = False):
        """`pipelined` (with `adaptive`; default False: the call sequence of RDyAdvance, unchanged): advance() ends with the
        operator's diagnostics_begin() instead of the blocking update_diagnostics(), and the NEXT advance() applies the forcing
        first -- RDyApplyForcing takes the time only -- and only then collects: diagnostics_wait(), reduce_courant() across
        ranks, the dt rule; then reset_diagnostics() and the steps.  The host so prepares interval k + 1 while the device
        finishes interval k.  The dt sequence, and with it the trajectory, is the same bits.  `max_courant` and `courant`
        collect on first access (on several ranks that is a collective: read them on all ranks or on none), and finish()
        collects at the end of a run.  Without `adaptive` no diagnostics call is made at all.
        `series`: a TimeSeries, or None (the default): none of the operator's series calls is made.  With one, the stepper
        plays WriteTimeSeries (src/time_series.c:530-564): one monitor call before the first step of its life (step 0) and one
        after every step, each doing, in this order,
          1. observations: if observation_interval is nonzero and step % observation_interval == 0, a record of the current
             state (after a fused Euler step: the step's output array).  The reference never advances observations.last_step,
             so there is no guard against a repeated step here either;
          2. if the boundary series is on, add_time(dt) with the INTERVAL's dt (rdy->dt, src/time_series.c:467), also after a
             last step that was shortened -- while the kernels accumulate dt x flux with the step's own h: the reference's
             arithmetic, kept;
          3. if step % boundary_flux_interval == 0 and step > last_step: a boundary-flux record, and last_step = step.
        The record times are the stepper's `time`.  series_read() returns a log.
        `means`: which time-averaged output fields to keep (OUTPUT_SOLUTION | OUTPUT_PRIMITIVE_VARIABLES | OUTPUT_SOURCES of
        rdycore_amd.operator; 0: none, and none of the operator's output-mean calls is made).  With bits set the stepper
        accumulates once before the first step of its life -- the initial state, whatever the primitive variables and the
        sources hold then -- and once after every step.  Every accumulate is weighted with the INTERVAL's dt, also after a
        last step that was shortened to land on the interval's end: the reference does the same
        (AccumulateOutputVar(.., rdy->dt), src/xdmf_output.c:452-456).  output_mean() returns a mean and starts a new window."""
        if temporal not in ("euler", "rk4"):
            raise ValueError(f"temporal = {temporal!r}: the explicit path has euler and rk4 (include/private/rdyconfigimpl.h:110-115)")
        self.temporal = temporal
        self._stage = None           # rk4: the stage state (local size) and k1..k4 (owned rows)
        self.op = op
        self.forcing = forcing   # rdycore_amd.forcing.Forcing: applied at the start of every interval, as the
                                 # driver calls RDyApplyForcing before each RDyAdvance (driver/main.c time loop)
        self.fused = fused
        self._u2 = None
        self.halo = halo
        # the stepper owns the two state arrays of the fused Euler step between the steps of one advance(): the pack of each
        # exchange can ride on the previous step's kernel (rdyhip_halo_fuse_pack); advance() invalidates at its start
        if halo is not None and fused and temporal == "euler" and getattr(halo, "_halo", None) is not None:
            halo.fuse_pack(True)
        self.adaptive = adaptive
        self.time = 0.0
        self.step = 0
        self.pipelined = bool(pipelined)
        self._pending = None         # pipelined: the device of a diagnostics_begin() that has not been collected yet
        self._max_courant = None     # diagnostics of the last interval, all ranks (None = not updated yet)
        self._courant = None         # the whole struct (value + global edge / cell id of the maximum)
        self._f = None
        self.means = int(means)
        if self.means:
            op.enable_output_means(self.means)
        self.series = series
        self._series_last_step = -1   # boundary_fluxes.last_step (InitBoundaryFluxes)
        if series is not None:
            if series.observation_interval:
                op.enable_observation_series(series.observation_sites, series.capacity)
            if series.boundary_flux_interval:
                op.enable_boundary_flux_series(series.capacity, series.boundaries)

    def _collect(self):
        """pipelined: the second half of UpdateOperatorDiagnostics for the read the last advance() began, if any"""
        if self._pending is None:
            return
        device, self._pending = self._pending, None
        self.op.diagnostics_wait()
        self._courant = reduce_courant(self.op.get_diagnostics(), device)
        self._max_courant = self._courant.max_courant_num

    def finish(self):
        """collects the diagnostics of the last interval of a run (pipelined; otherwise there is nothing left to collect)"""
        self._collect()

    @property
    def max_courant(self):
        self._collect()
        return self._max_courant

    @property
    def courant(self):
        self._collect()
        return self._courant

    def _series_monitor(self, dt, state):
        """WriteTimeSeries(ts, step, time, X) for the step count and time the stepper stands at"""
        from .operator import SERIES_BOUNDARY_FLUXES, SERIES_OBSERVATIONS
        s = self.series
        if s.observation_interval and self.step % s.observation_interval == 0:
            self.op.series_record(SERIES_OBSERVATIONS, self.time, state)
        if s.boundary_flux_interval:
            self.op.series_add_time(dt)
            if self.step % s.boundary_flux_interval == 0 and self.step > self._series_last_step:
                self.op.series_record(SERIES_BOUNDARY_FLUXES, self.time)
                self._series_last_step = self.step

    def series_read(self, kind: int, clear: bool = False):
        """the log of one series, (times, values [records, entries, 3]); `clear`: the log then starts empty"""
        out = self.op.series_read(kind)
        if clear:
            self.op.series_clear(kind)
        return out

    def output_mean(self, var: int):
        """ComputeMean + ResetOutputVar (src/xdmf_output.c:211-241) of one variable: (mean [owned,3], accumulated time); the
        variable's next window starts empty"""
        mean, t = self.op.output_mean(var)
        self.op.reset_output_means(var)
        return mean, t

    def rhs(self, dt, u_local, f_global):
        if self.halo is not None and self.halo.world > 1:
            self.halo.rhs_overlapped(self.op, dt, u_local, f_global)
        else:
            self.op.rhs_function(dt, u_local, f_global)

    def advance(self, u_local: torch.Tensor, dt: float, interval: float) -> float:
        """RDyAdvance: integrate from self.time to self.time + interval; returns
        the dt to use next (changed only by adaptive stepping)."""
        if self._f is None or self._f.shape[0] != self.op.mesh.num_owned_cells:
            self._f = torch.empty((self.op.mesh.num_owned_cells, 3), dtype=torch.float64, device=u_local.device)
        a = self.adaptive
        if self.pipelined and self.forcing is not None:
            self.forcing.apply(self.time)       # nothing in it depends on dt: staged while the device finishes the last interval
        self._collect()
        cmax = self._max_courant
        if a is not None and cmax is not None:
            # src/rdyadvance.c:308-330: rescaled whenever the diagnostics are valid; a zero Courant number (nothing
            # wet) makes target / max infinite there, i.e. the factor is max_increase_factor
            if cmax < a.target_courant_number:
                ratio = a.target_courant_number / cmax if cmax > 0.0 else float("inf")
                dt *= min(ratio, a.max_increase_factor)
                dt = min(dt, interval)
            else:
                dt *= a.target_courant_number / cmax
        t_end = self.time + interval
        if self.forcing is not None and not self.pipelined:
            self.forcing.apply(self.time)
        self.op.reset_diagnostics()
        if self.halo is not None and getattr(self.halo, "_halo", None) is not None:
            self.halo.invalidate()          # the caller may have written u_local since the last interval
        cur = u_local
        if self.fused and (self._u2 is None or self._u2.shape != u_local.shape):
            self._u2 = torch.empty_like(u_local)
        m = self.means
        if m and self.step == 0:
            self.op.accumulate_output_means(m, dt, u_local)      # the monitor's call at step 0
        if self.series is not None and self.step == 0:
            self._series_monitor(dt, u_local)
        while self.time < t_end * (1.0 - 1e-14):
            h = min(dt, t_end - self.time)       # TS_EXACTFINALTIME_MATCHSTEP
            if self.temporal == "rk4":
                self._rk4_step(h, u_local)
                if m:
                    self.op.accumulate_output_means(m, dt, u_local)
            elif self.fused:
                nxt = self._u2 if cur is u_local else u_local
                if self.halo is not None and self.halo.world > 1:
                    self.halo.step_overlapped(self.op, h, cur, nxt)
                else:
                    self.op.euler_step(h, cur, nxt)   # resets the Courant diagnostic like every RHS (src/rdysetup.c:1136)
                cur = nxt
                if m:
                    self.op.accumulate_output_means(m, dt, nxt)   # solution: the step's output; primitive variables: of its input
            else:
                self.rhs(h, u_local, self._f)
                if m & 6:
                    # the primitive variables belong to the state the RHS saw: before the axpy rewrites it in place
                    self.op.accumulate_output_means(m & 6, dt)
                self.op.axpy_owned(h, self._f, u_local)
                if m & 1:
                    self.op.accumulate_output_means(1, dt, u_local)
            self.time += h
            self.step += 1
            if self.series is not None:
                self._series_monitor(dt, cur if self.temporal == "euler" and self.fused else u_local)
        if cur is not u_local:
            u_local.copy_(cur)                   # an odd number of steps ended in the second buffer (euler, fused)
        if a is not None and self.pipelined:
            self.op.diagnostics_begin()          # collected by the next advance(), by finish() or on first access
            self._pending = u_local.device
        elif a is not None:
            # UpdateOperatorDiagnostics: local 16-byte copy + the MPI_Allreduce(max) of src/operator.c:879
            self.op.update_diagnostics()
            self._courant = reduce_courant(self.op.get_diagnostics(), u_local.device)
            self._max_courant = self._courant.max_courant_num
        return dt

    def _rk4_step(self, h: float, u_local: torch.Tensor):
        """TSStep_RK with the TSRK4 tableau (A = [[0], [1/2], [0, 1/2], [0, 0, 1]], b = [1/6, 1/3, 1/3, 1/6]): every stage
        is one OperatorRHSFunction on the stage state; the diagnostics left behind are the last stage's, as in the reference"""
        if self.fused and hasattr(self.op, "rk4_step"):
            # the whole step behind the C ABI, unless the ghost update is driven from Python (transport="torch")
            if self.halo is None or self.halo.world == 1:
                return self.op.rk4_step(h, u_local)
            if getattr(self.halo, "_halo", None) is not None:
                return self.op.rk4_step(h, u_local, halo=self.halo)
        no = self.op.mesh.num_owned_cells
        if self._stage is None or self._stage[0].shape != u_local.shape:
            self._stage = [torch.empty_like(u_local)] + [torch.empty((no, 3), dtype=torch.float64, device=u_local.device) for _ in range(4)]
        y, k = self._stage[0], self._stage[1:]
        self.rhs(h, u_local, k[0])
        for j, a in ((1, 0.5), (2, 0.5), (3, 1.0)):
            y.copy_(u_local)                       # ghost rows are refreshed by the stage's own exchange
            self.op.axpy_owned(a * h, k[j - 1], y)
            self.rhs(h, y, k[j])
        for j, b in enumerate((1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)):
            self.op.axpy_owned(b * h, k[j], u_local)


class EnsembleEulerStepper:
    """Forward Euler for an operator with the ensemble enabled (Operator.enable_ensemble): every member takes the same number of
    steps, member m with its own fixed dts[m], one fused launch per step for all members (rdyhip_ensemble_euler_step), the
    steps ping-ponging between two [B, num_cells, 3] arrays.  Adaptive per-member dt is a follow-up."""

    def __init__(self, op, means: int = 0, series: Optional[TimeSeries] = None):
        """`means` (OUTPUT_* bits; 0, the default: none of the operator's ensemble output-mean calls is made): the stepper enables
        the [B, owned, 3] accumulators and, after every step, accumulates with solution = the step's output and primitive
        variables = the step's input state, member m weighted with the step's dts[m], one launch for all members.  `series` (a
        TimeSeries; None, the default: no series call is made): its observation sites are enabled, and after every step whose
        count is a multiple of observation_interval a record of the step's output is appended at the members' times.  There is
        no boundary-flux series for ensembles, and -- as with TracerEulerStepper -- no monitor call before the first step."""
        self.op = op
        self.step = 0
        self.times = None        # [B] the time every member has reached
        self._own = [None, None]  # the stepper's arrays: the partner of the caller's array, and the partner of that one
        self.means = int(means)
        if self.means:
            op.ensemble_enable_output_means(self.means)
        self.series = series
        if series is not None and series.observation_interval:
            op.ensemble_enable_observation_series(series.observation_sites, series.capacity)

    def _partner(self, u: torch.Tensor) -> torch.Tensor:
        """the array the first step from `u` writes: the stepper's first array, or -- when `u` is one of the stepper's own, the
        result of an earlier advance handed back -- its other one.  Never `u`, and never an array of the caller's."""
        k = 1 if self._own[0] is u else 0
        a = self._own[k]
        if a is None or a.shape != u.shape or a.device != u.device:
            a = self._own[k] = u.clone()     # ghost rows start as u's
        return a

    def advance(self, u: torch.Tensor, dts, nsteps: int) -> torch.Tensor:
        """`nsteps` steps from `u`; returns the array that holds the result: `u` after an even number of steps, else one of the
        stepper's own two arrays (a later advance overwrites it: copy what must be kept), which may be handed back as the next
        `u`.  No array of the caller's other than `u` is written.  Ghost rows are the caller's: a rank with
        ghost cells exchanges every member's slice of the returned array between calls."""
        d = np.ascontiguousarray(dts, dtype=np.float64).ravel()
        if self.times is None:
            self.times = np.zeros(d.size)
        cur, nxt = u, self._partner(u)
        s = self.series
        for _ in range(int(nsteps)):
            self.op.ensemble_euler_step(d, cur, nxt)
            if self.means:
                self.op.ensemble_accumulate_output_means(self.means, d, nxt, cur)   # solution: the step's output; primitive: its input
            cur, nxt = nxt, cur
            self.times = self.times + d
            self.step += 1
            if s is not None and s.observation_interval and self.step % s.observation_interval == 0:
                self.op.ensemble_series_record(self.times, cur)
        return cur

    def series_read(self, clear: bool = False):
        """the observation log, (times [records, B], values [records, B, sites, 3]); `clear`: the log then starts empty"""
        out = self.op.ensemble_series_read()
        if clear:
            self.op.ensemble_series_clear()
        return out

    def output_mean(self, var: int):
        """(means [B, owned, 3], accumulated times [B]) of one variable; its next window starts empty"""
        mean, t = self.op.ensemble_output_mean(var)
        self.op.ensemble_reset_output_means(var)
        return mean, t


class TracerEulerStepper:
    """Forward Euler for an operator with tracers enabled (Operator.enable_tracers): fused Euler steps
    (rdyhip_tracers_euler_step: the update rides on the kernel's stores) ping-ponging between two [num_cells, 3 + NT] arrays.
    With a `halo` (HaloExchange, transport="c") every step is HaloExchange.tracers_step_overlapped -- the ghost update of the
    3 + NT-wide state and the step in one call -- so only the owned rows of the arrays need to be current between steps."""

    def __init__(self, op, halo=None, means: int = 0, series: Optional[TimeSeries] = None):
        """`means` (OUTPUT_* bits; 0, the default: none of the operator's tracer output-mean calls is made): the stepper enables
        the [owned, 3 + NT] accumulators and, after every step, accumulates with solution = the step's output and primitive
        variables = the step's input state, weighted with the step's dt.  `series` (a TimeSeries; None, the default: no series
        call is made): its observation sites are enabled, and after every step whose count is a multiple of
        observation_interval a record of the step's output is appended at the stepper's time.  There is no boundary-flux series
        for tracers, and -- unlike EulerStepper -- no monitor call before the first step."""
        self.op = op
        self.halo = halo
        self.step = 0
        self.time = 0.0
        self._own = [None, None]  # the stepper's arrays: the partner of the caller's array, and the partner of that one
        self.means = int(means)
        if self.means:
            op.tracers_enable_output_means(self.means)
        self.series = series
        if series is not None and series.observation_interval:
            op.tracers_enable_observation_series(series.observation_sites, series.capacity)

    def _partner(self, u: torch.Tensor) -> torch.Tensor:
        """as EnsembleEulerStepper._partner: never `u`, never another array of the caller's"""
        k = 1 if self._own[0] is u else 0
        a = self._own[k]
        if a is None or a.shape != u.shape or a.device != u.device:
            a = self._own[k] = u.clone()     # ghost rows start as u's
        return a

    def advance(self, u: torch.Tensor, dt: float, nsteps: int) -> torch.Tensor:
        """`nsteps` steps of `dt` from `u`; returns the array that holds the result: `u` after an even number of steps, else one
        of the stepper's own two arrays (a later advance overwrites it), which may be handed back as the next `u`.  The caller
        sets sources and boundary values between calls.  With a halo the ghost rows of the returned array are one step old
        (or the caller's): the next step's exchange fills them."""
        cur, nxt = u, self._partner(u)
        for _ in range(int(nsteps)):
            if self.halo is not None:
                self.halo.tracers_step_overlapped(self.op, dt, cur, nxt)
            else:
                self.op.tracers_euler_step(dt, cur, nxt)
            if self.means:
                self.op.tracers_accumulate_output_means(self.means, dt, nxt, cur)   # solution: the step's output; primitive: its input
            cur, nxt = nxt, cur
            self.time += dt
            self.step += 1
            s = self.series
            if s is not None and s.observation_interval and self.step % s.observation_interval == 0:
                self.op.tracers_series_record(self.time, cur)
        return cur

    def series_read(self, clear: bool = False):
        """the observation log, (times, values [records, sites, 3 + NT]); `clear`: the log then starts empty"""
        out = self.op.tracers_series_read()
        if clear:
            self.op.tracers_series_clear()
        return out

    def output_mean(self, var: int):
        """(mean [owned, 3 + NT], accumulated time) of one variable; its next window starts empty"""
        mean, t = self.op.tracers_output_mean(var)
        self.op.tracers_reset_output_means(var)
        return mean, t
