// Shallow water with advected tracers behind the C ABI (rdyhip_tracers_*, rdyhip_tracer_hr_*; kernels: tracer_kernels.h): the
// choice among the 28 instantiations of either family (plain / hydrostatic reconstruction), the launch, the two enables and the
// setters / getters of what only this path has.  Included by rdyhip_api.hip only.
#pragma once
namespace {

using TracerKernelFn = void (*)(const KernelArgs, const TracerArgs, const double, const double *);

// The instantiation of the tracer kernel for (family: hydrostatic reconstruction (rdyhip_tracer_hr_enable) or plain, slots per
// cell, number of tracers, upwind tracer flux): 2 x (2 x 7 x 2) = 56
TracerKernelFn tracer_kernel_fn(bool hr, int S, int nt, bool upwind) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(upwind, [&](auto up) { return with_tracer_count(nt, [&](auto n) -> TracerKernelFn {
    constexpr int s = quad ? 4 : 3, t = decltype(n)::value;
    return hr ? tracer_hr_kernel<s, t, up> : tracer_rhs_kernel<s, t, up>;
  }); }); });
}

// null operator, tracers not enabled: what every call after rdyhip_tracers_enable starts with
int tracers_check(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->tracers.n == 0) return fail(RDYHIP_ERR_USER, "tracers are not enabled (rdyhip_tracers_enable)");
  return 0;
}

// One tracer evaluation: OperatorRHSFunction's zeroing of F, diagnostics reset and apply in one launch; with u_out the
// forward-Euler update rides on the stores (f may then be NULL)
// Phased (rdyhip_tracer_phase_*, the halo steps below): every phase is a launch over ALL owned cells whose threads of the
// other phase stand aside (tracer_kernels.h), so a workgroup keeps its Courant bucket from phase to phase; reset == 0 merges
// into the buckets.  A HALO phase on a rank without ghost-adjacent cells launches nothing (with `reset` the buckets are
// still restarted, as step_two_streams does for the SWE path).
int launch_tracers(RDyHipOperator op, double dt, const double *u, double *f, double *u_out, hipStream_t st, int32_t phase = RDYHIP_PHASE_ALL,
                   bool reset = true) {
  if (op->n_owned == 0) return 0;   // a rank may own nothing: nothing to launch
  if (reset) op->courant = RDyHipCourant{0.0, -1, -1};
  if (phase == RDYHIP_PHASE_HALO && op->n_halo == 0) {
    if (reset) {
      const int rc = rdyhip_reset_diagnostics(op, (void *)st);
      if (rc) return rc;
    }
    op->courant_owned_side = true;
    return 0;
  }
  op->courant_owned_side = true;   // rdyhip_update_diagnostics: the cell of a cut edge is the owned one
  KernelArgs a = kernel_args_all_cells(op);
  a.mannings   = op->d_mannings.p;
  a.extsrc     = op->d_extsrc.p;   // the canonical [owned][3] array, whatever the water-only mode of the SWE kernels says
  a.src_mom    = 1;
  a.n_buckets  = (int32_t)op->d_blk_max.n;
  a.reset_diag = reset ? 1 : 0;
  a.phase      = phase;
  TracerArgs t{};
  t.bvalues = op->tracers.bvalues.p;
  t.bflux   = op->tracers.bflux.p;
  t.src     = op->tracers.src.p;
  t.pv      = op->tracers.pv_wanted ? op->tracers.pv.p : nullptr;   // read here, when the launch is enqueued
  t.f       = f;
  t.u_out   = u_out;
  const bool upwind = op->tracers.riemann == RDYHIP_TRACER_RIEMANN_UPWIND_ROE;
  // kernel_args_all_cells carries the slot tables (every operator has them) but not the bed elevations of an HR operator
  if (op->tracers.hr) a.zc_local = op->d_zc_local.p;
  TracerKernelFn kfn = tracer_kernel_fn(op->tracers.hr, op->S, op->tracers.n, upwind);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(op->grid), dim3(BLOCK), 0, st, a, t, dt, u);
  HIP_TRY(hipGetLastError());
  return 0;
}

// what a phased call checks beyond tracers_check: the phase and the flags (RDYHIP_PHASE_OVERWRITE is implied and accepted)
int tracer_phase_check(int32_t phase, int32_t flags) {
  if (phase != RDYHIP_PHASE_ALL && phase != RDYHIP_PHASE_INTERIOR && phase != RDYHIP_PHASE_HALO) return fail(RDYHIP_ERR_USER, "unknown phase %d", phase);
  if (flags & ~(RDYHIP_PHASE_OVERWRITE | RDYHIP_PHASE_RESET_DIAGNOSTICS))
    return fail(RDYHIP_ERR_USER, "unknown flags %d (the tracer phases take RDYHIP_PHASE_RESET_DIAGNOSTICS only; there is no accumulate form)", flags);
  return 0;
}

// ---- the ghost update of the [num_cells][3 + NT] state and the evaluation in one call (rdyhip_halo_tracers_*) --------------
// A halo created before rdyhip_tracers_enable has buffers of 3 (6) values per cell: the first tracer step makes them
// 3 + NT wide.  The only place of the tracer path that waits for the device: what the halo's stream and the caller's still
// run may read the old buffers.  The fused pack's send lists point into d_send and are attached again.
int halo_grow(RDyHipHalo h, int32_t ncomp, hipStream_t st) {
  if (ncomp <= h->max_comp) return 0;
  HIP_TRY(hipStreamSynchronize(h->cs));
  HIP_TRY(hipStreamSynchronize(st));
  int rc      = h->d_send.zeros((size_t)h->send_off.back() * ncomp);
  if (!rc) rc = h->d_recv.zeros((size_t)h->recv_off.back() * ncomp);
  if (rc) return rc;
  h->max_comp     = ncomp;
  h->packed_state = nullptr;
  if (h->fused_pack && h->op->fused_halo == h) return halo_attach_send_lists(h, true);
  return 0;
}

// In order: pack, transfer, unpack of 3 + NT values per cell on the caller's stream, then ONE launch over all owned cells
int tracer_step_in_order(RDyHipOperator op, RDyHipHalo h, int32_t N, double dt, double *u, double *f, double *u_out, hipStream_t st) {
  int rc      = halo_pack(h, u, N, st);
  if (!rc) rc = halo_transfer(h, u, N, st);
  if (!rc) rc = halo_unpack(h, u, N, st);
  if (!rc) rc = launch_tracers(op, dt, u, f, u_out, st);
  return rc;
}

// Two streams, the simple shape of step_two_streams: the exchange on the halo's stream, the INTERIOR launch (which starts the
// diagnostic) on the caller's meanwhile -- enqueued before a transport callback that may block the host, behind an
// asynchronous RCCL group --, the join, then the HALO launch (which merges into the buckets) on the caller's stream too
int tracer_step_two_streams(RDyHipOperator op, RDyHipHalo h, int32_t N, double dt, double *u, double *f, double *u_out, hipStream_t st) {
  h->next_events();
  HIP_TRY(hipEventRecord(h->ev_fork, st));
  HIP_TRY(hipStreamWaitEvent(h->cs, h->ev_fork, 0));
  int rc = halo_pack(h, u, N, h->cs);
  if (!rc && h->transport) rc = launch_tracers(op, dt, u, f, u_out, st, RDYHIP_PHASE_INTERIOR, true);
  if (!rc) rc = halo_transfer(h, u, N, h->cs);
  if (!rc) rc = halo_unpack(h, u, N, h->cs);
  if (!rc && !h->transport) rc = launch_tracers(op, dt, u, f, u_out, st, RDYHIP_PHASE_INTERIOR, true);
  // an error after the fork still joins the exchange stream back (step_two_streams)
  hipError_t e = hipEventRecord(h->ev_join, h->cs);
  if (e == hipSuccess) e = hipStreamWaitEvent(st, h->ev_join, 0);
  if (rc) return rc;
  if (e != hipSuccess) return fail(RDYHIP_ERR_LIB, "joining the exchange stream failed: %s", hipGetErrorString(e));
  return launch_tracers(op, dt, u, f, u_out, st, RDYHIP_PHASE_HALO, false);
}

// rdyhip_halo_tracers_rhs (euler == false) / rdyhip_halo_tracers_euler_step
int tracers_overlapped(RDyHipOperator op, RDyHipHalo h, bool euler, double dt, double *u, double *f, double *u_out, hipStream_t st) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!h) return fail(RDYHIP_ERR_USER, "null halo");
  if (h->op != op) return fail(RDYHIP_ERR_USER, "the halo belongs to another operator");
  if (op->n_cells > 0 && !u) return fail(RDYHIP_ERR_USER, "null u_local");
  if (euler) {
    if (u_out == u && u) return fail(RDYHIP_ERR_USER, "rdyhip_halo_tracers_euler_step needs a second state array (not in place)");
    rc = euler_out_check(op, "rdyhip_halo_tracers_euler_step", u, u_out);
    if (rc) return rc;
  } else if (op->n_owned > 0 && !f) {
    return fail(RDYHIP_ERR_USER, "null f_global");
  }
  const int32_t N = 3 + op->tracers.n;
  rc = halo_grow(h, N, st);
  if (!rc) rc = halo_check(h, u, N);
  if (rc) return rc;
  op->courant            = RDyHipCourant{0.0, -1, -1};
  op->courant_owned_side = true;
  const int kind = euler ? RDYHIP_HALO_STEP_TRACERS_EULER : RDYHIP_HALO_STEP_TRACERS_RHS;
  int       slot = -1;
  int       form = form_begin(h, kind, st, &slot);
  if (h->tracers_in_order) form = 0;
  rc = form ? tracer_step_two_streams(op, h, N, dt, u, f, u_out, st) : tracer_step_in_order(op, h, N, dt, u, f, u_out, st);
  form_end(h, kind, st, slot);
  h->packed_state = nullptr;   // d_send holds 3 + NT-wide rows: a later rdyhip_euler_step_overlapped packs again
  return rc;
}

}  // namespace

extern "C" int rdyhip_tracer_phase_rhs(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *f_global, void *stream) {
  int rc = tracers_check(op);
  if (!rc) rc = tracer_phase_check(phase, flags);
  if (rc) return rc;
  if (op->n_owned > 0 && (!u_local || !f_global)) return fail(RDYHIP_ERR_USER, "null u_local / f_global");
  return launch_tracers(op, dt, u_local, f_global, nullptr, (hipStream_t)stream, phase, (flags & RDYHIP_PHASE_RESET_DIAGNOSTICS) != 0);
}

extern "C" int rdyhip_tracer_phase_euler_step(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *u_local_out,
                                              double *f_global, void *stream) {
  int rc = tracers_check(op);
  if (!rc) rc = tracer_phase_check(phase, flags);
  if (rc) return rc;
  if (op->n_owned > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  rc = euler_out_check(op, "rdyhip_tracer_phase_euler_step", u_local, u_local_out);
  if (rc) return rc;
  return launch_tracers(op, dt, u_local, f_global, u_local_out, (hipStream_t)stream, phase, (flags & RDYHIP_PHASE_RESET_DIAGNOSTICS) != 0);
}

extern "C" int rdyhip_halo_tracers_rhs(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, double *f_global, void *stream) {
  return tracers_overlapped(op, halo, false, dt, u_local, f_global, nullptr, (hipStream_t)stream);
}

extern "C" int rdyhip_halo_tracers_euler_step(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, double *u_local_out, double *f_global,
                                              void *stream) {
  return tracers_overlapped(op, halo, true, dt, u_local, f_global, u_local_out, (hipStream_t)stream);
}

// rdyhip_tracers_enable (hr == false) / rdyhip_tracer_hr_enable (hr == true): the checks in the order the header lists them, then
// the allocations -- the same for both
static int tracers_enable(RDyHipOperator op, int32_t num_tracers, int32_t riemann, bool hr) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->tracers.n != 0)
    return fail(RDYHIP_ERR_USER, "tracers are already enabled (%d%s)", op->tracers.n, op->tracers.hr ? ", hydrostatic reconstruction" : "");
  if (num_tracers < 1 || num_tracers > RDYHIP_MAX_TRACERS)
    return fail(RDYHIP_ERR_USER, "num_tracers (%d) must be in 1..%d", num_tracers, RDYHIP_MAX_TRACERS);
  if (riemann != RDYHIP_TRACER_RIEMANN_ROE && riemann != RDYHIP_TRACER_RIEMANN_UPWIND_ROE)
    return fail(RDYHIP_ERR_USER, "unknown tracer Riemann solver %d", riemann);
  if (op->muscl || op->config.second_order) return fail(RDYHIP_ERR_USER, "tracers are first order only (the operator was created with second_order)");
  const bool op_hr = op->hr || op->config.well_balancing != RDYHIP_WELL_BALANCING_NONE;
  if (!hr && op_hr)
    return fail(RDYHIP_ERR_USER, "rdyhip_tracers_enable is for operators without well balancing (well_balancing = %d): use rdyhip_tracer_hr_enable",
                op->config.well_balancing);
  if (hr && !(op->hr && op->config.well_balancing == RDYHIP_WELL_BALANCING_HR))
    return fail(RDYHIP_ERR_USER, "rdyhip_tracer_hr_enable needs an operator created with RDYHIP_WELL_BALANCING_HR (well_balancing = %d): use rdyhip_tracers_enable",
                op->config.well_balancing);
  if (op->config.source_method != RDYHIP_SOURCE_SEMI_IMPLICIT)
    return fail(RDYHIP_ERR_USER, hr ? "Only semi_implicit is supported for tracer HR (source_method = %d)"   // tracer_petsc.c:1191
                                    : "tracers have the semi-implicit source only (source_method = %d)", op->config.source_method);
  for (size_t k = 0; k < op->h_btype.size(); ++k)
    if (op->h_btype[k] == RDYHIP_CONDITION_CRITICAL_OUTFLOW)
      return fail(RDYHIP_ERR_USER, "CONDITION_CRITICAL_OUTFLOW not supported for tracers");   // tracer_petsc.c:472-474
    else if (op->h_btype[k] != RDYHIP_CONDITION_DIRICHLET && op->h_btype[k] != RDYHIP_CONDITION_REFLECTING)
      return fail(RDYHIP_ERR_USER, "Invalid boundary condition %d encountered for tracers", op->h_btype[k]);
  const size_t N = 3 + (size_t)num_tracers, K = (size_t)op->K, no = (size_t)op->n_owned;
  TracerState t;
  int rc = t.bvalues.zeros(N * K);
  if (!rc) rc = t.bflux.zeros(N * K);
  if (!rc) rc = t.src.zeros((size_t)num_tracers * no);
  if (rc) return rc;
  t.n         = num_tracers;
  t.riemann   = riemann;
  t.hr        = hr;
  op->tracers = std::move(t);
  return 0;
}

extern "C" int rdyhip_tracers_enable(RDyHipOperator op, int32_t num_tracers, int32_t riemann) { return tracers_enable(op, num_tracers, riemann, false); }

extern "C" int rdyhip_tracer_hr_enable(RDyHipOperator op, int32_t num_tracers, int32_t riemann) { return tracers_enable(op, num_tracers, riemann, true); }

extern "C" int rdyhip_tracer_hr_info(RDyHipOperator op, int32_t *well_balancing) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (well_balancing) *well_balancing = op->tracers.n != 0 && op->tracers.hr ? RDYHIP_WELL_BALANCING_HR : RDYHIP_WELL_BALANCING_NONE;
  return 0;
}

extern "C" int rdyhip_tracers_info(RDyHipOperator op, int32_t *num_tracers, int32_t *riemann) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (num_tracers) *num_tracers = op->tracers.n;
  if (riemann) *riemann = op->tracers.riemann;
  return 0;
}

extern "C" int rdyhip_tracers_set_boundary_values(RDyHipOperator op, int32_t boundary, int32_t num_edges, const double *values) {
  int rc = tracers_check(op);
  if (rc) return rc;
  return boundary_rows_copy(op, boundary, num_edges, op->tracers.bvalues.p, 3 + (size_t)op->tracers.n, const_cast<double *>(values), true);
}

extern "C" int rdyhip_tracers_set_source(RDyHipOperator op, int32_t tracer, int32_t n, const int32_t *owned_cell_ids, const double *values) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (tracer < 0 || tracer >= op->tracers.n) return fail(RDYHIP_ERR_USER, "tracer index %d out of range (%d tracers)", tracer, op->tracers.n);
  return scatter_component(op, op->tracers.src.p, op->tracers.n, tracer, n, owned_cell_ids, values);
}

extern "C" int rdyhip_tracers_rhs_function(RDyHipOperator op, double dt, const double *u_local, double *f_global, void *stream) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (op->n_owned > 0 && (!u_local || !f_global)) return fail(RDYHIP_ERR_USER, "null u_local / f_global");
  return launch_tracers(op, dt, u_local, f_global, nullptr, (hipStream_t)stream);
}

extern "C" int rdyhip_tracers_euler_step(RDyHipOperator op, double dt, const double *u_local, double *u_local_out, double *f_global, void *stream) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (op->n_owned > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  rc = euler_out_check(op, "rdyhip_tracers_euler_step", u_local, u_local_out);
  if (rc) return rc;
  return launch_tracers(op, dt, u_local, f_global, u_local_out, (hipStream_t)stream);
}

extern "C" int rdyhip_tracers_primitive_variables(RDyHipOperator op, const double **device_ptr, int64_t *num_values) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!device_ptr) return fail(RDYHIP_ERR_USER, "null argument");
  const size_t n = (3 + (size_t)op->tracers.n) * (size_t)op->n_owned;
  if (!op->tracers.pv.p) {
    DevBuf<double> pv;
    rc = pv.zeros(n);
    if (rc) return rc;
    op->tracers.pv = std::move(pv);
  }
  op->tracers.pv_wanted = true;
  *device_ptr = op->tracers.pv.p;
  if (num_values) *num_values = (int64_t)n;
  return 0;
}

extern "C" int rdyhip_tracers_get_boundary_fluxes(RDyHipOperator op, int32_t boundary, int32_t num_edges, double *fluxes) {
  int rc = tracers_check(op);
  if (rc) return rc;
  return boundary_rows_copy(op, boundary, num_edges, op->tracers.bflux.p, 3 + (size_t)op->tracers.n, fluxes, false);
}

