// Shallow water with advected tracers behind the C ABI (rdyhip_tracers_*; kernel: tracer_kernels.h): the choice among the 28
// instantiations, the launch, enable and the setters / getters of what only this path has.  Included by rdyhip_api.hip only.
#pragma once
namespace {

using TracerKernelFn = void (*)(const KernelArgs, const TracerArgs, const double, const double *);

// The instantiation of the tracer kernel for (slots per cell, number of tracers, upwind tracer flux): 2 x 7 x 2 = 28
template <int S, bool UPWIND>
TracerKernelFn tracer_kernel_nt(int nt) {
  switch (nt) {
    case 1: return tracer_rhs_kernel<S, 1, UPWIND>;
    case 2: return tracer_rhs_kernel<S, 2, UPWIND>;
    case 3: return tracer_rhs_kernel<S, 3, UPWIND>;
    case 4: return tracer_rhs_kernel<S, 4, UPWIND>;
    case 5: return tracer_rhs_kernel<S, 5, UPWIND>;
    case 6: return tracer_rhs_kernel<S, 6, UPWIND>;
    default: return tracer_rhs_kernel<S, 7, UPWIND>;
  }
}
TracerKernelFn tracer_kernel_fn(int S, int nt, bool upwind) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(upwind, [&](auto up) -> TracerKernelFn {
    return tracer_kernel_nt<quad ? 4 : 3, up>(nt);
  }); });
}

// null operator, tracers not enabled: what every call after rdyhip_tracers_enable starts with
int tracers_check(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->tracers.n == 0) return fail(RDYHIP_ERR_USER, "tracers are not enabled (rdyhip_tracers_enable)");
  return 0;
}

// One tracer evaluation: OperatorRHSFunction's zeroing of F, diagnostics reset and apply in one launch; with u_out the
// forward-Euler update rides on the stores (f may then be NULL)
int launch_tracers(RDyHipOperator op, double dt, const double *u, double *f, double *u_out, hipStream_t st) {
  if (op->n_owned == 0) return 0;   // a rank may own nothing: nothing to launch
  op->courant = RDyHipCourant{0.0, -1, -1};
  op->courant_owned_side = true;   // rdyhip_update_diagnostics: the cell of a cut edge is the owned one
  KernelArgs a = kernel_args_all_cells(op);
  a.mannings   = op->d_mannings.p;
  a.extsrc     = op->d_extsrc.p;   // the canonical [owned][3] array, whatever the water-only mode of the SWE kernels says
  a.src_mom    = 1;
  a.n_buckets  = (int32_t)op->d_blk_max.n;
  a.reset_diag = 1;
  TracerArgs t{};
  t.bvalues = op->tracers.bvalues.p;
  t.bflux   = op->tracers.bflux.p;
  t.src     = op->tracers.src.p;
  t.pv      = op->tracers.pv_wanted ? op->tracers.pv.p : nullptr;   // read here, when the launch is enqueued
  t.f       = f;
  t.u_out   = u_out;
  TracerKernelFn kfn = tracer_kernel_fn(op->S, op->tracers.n, op->tracers.riemann == RDYHIP_TRACER_RIEMANN_UPWIND_ROE);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(op->grid), dim3(BLOCK), 0, st, a, t, dt, u);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int rdyhip_tracers_enable(RDyHipOperator op, int32_t num_tracers, int32_t riemann) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->tracers.n != 0) return fail(RDYHIP_ERR_USER, "tracers are already enabled (%d)", op->tracers.n);
  if (num_tracers < 1 || num_tracers > RDYHIP_MAX_TRACERS)
    return fail(RDYHIP_ERR_USER, "num_tracers (%d) must be in 1..%d", num_tracers, RDYHIP_MAX_TRACERS);
  if (riemann != RDYHIP_TRACER_RIEMANN_ROE && riemann != RDYHIP_TRACER_RIEMANN_UPWIND_ROE)
    return fail(RDYHIP_ERR_USER, "unknown tracer Riemann solver %d", riemann);
  if (op->muscl || op->config.second_order) return fail(RDYHIP_ERR_USER, "tracers are first order only (the operator was created with second_order)");
  if (op->hr || op->config.well_balancing != RDYHIP_WELL_BALANCING_NONE)
    return fail(RDYHIP_ERR_USER, "tracers with well balancing are not supported (well_balancing = %d)", op->config.well_balancing);
  if (op->config.source_method != RDYHIP_SOURCE_SEMI_IMPLICIT)
    return fail(RDYHIP_ERR_USER, "tracers have the semi-implicit source only (source_method = %d)", op->config.source_method);
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
  op->tracers = std::move(t);
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

