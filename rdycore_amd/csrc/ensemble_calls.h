// Ensembles behind the C ABI (rdyhip_ensemble_*, rdyhip_ens_hr_*; kernels: ensemble_kernels.h): B members on one mesh, one launch
// per evaluation of either family (plain / hydrostatic reconstruction); the two enables, the members' setters / getters and
// their Courant diagnostics.  Included by rdyhip_api.hip only.
#pragma once
namespace {

using EnsembleKernelFn = void (*)(const KernelArgs, const EnsembleArgs, const double *);

// The instantiation of the ensemble kernel for (family: hydrostatic reconstruction (rdyhip_ens_hr_enable) or plain, slots per
// cell, source method, the fused Euler update): 2 x (2 x 2 x 2) = 16
EnsembleKernelFn ensemble_kernel_fn(bool hr, int S, int src, bool euler) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(src != 0, [&](auto xq) { return with_flag(euler, [&](auto eu) -> EnsembleKernelFn {
    constexpr int s = quad ? 4 : 3, sm = xq ? 1 : 0;
    return hr ? ensemble_hr_kernel<s, sm, eu> : ensemble_rhs_kernel<s, sm, eu>;
  }); }); });
}

// null operator, ensemble not enabled: what every call after rdyhip_ensemble_enable starts with; then the member index
int ensemble_check(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->ensemble.members == 0) return fail(RDYHIP_ERR_USER, "the ensemble is not enabled (rdyhip_ensemble_enable)");
  return 0;
}
int ensemble_check_member(RDyHipOperator op, int32_t member) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (member < 0 || member >= op->ensemble.members) return fail(RDYHIP_ERR_USER, "member index %d out of range (%d members)", member, op->ensemble.members);
  return 0;
}

// One evaluation of all members: per member OperatorRHSFunction's zeroing of F, diagnostics reset and apply; with u_out the
// forward-Euler update rides on the stores (f may then be NULL)
int launch_ensemble(RDyHipOperator op, const double *dts, const double *u, double *f, double *u_out, hipStream_t st) {
  for (auto &c : op->ensemble.courant) c = RDyHipCourant{0.0, -1, -1};
  if (op->n_owned == 0) return 0;   // a rank may own nothing: nothing to launch
  KernelArgs a = kernel_args_all_cells(op);   // Manning's n, the source and the Courant buckets are the members' own
  // kernel_args_all_cells carries the slot tables (every operator has them) but not the bed elevations of an HR operator
  if (op->ensemble.hr) a.zc_local = op->d_zc_local.p;
  EnsembleArgs     t{};
  t.mannings  = op->ensemble.mannings.p;
  t.extsrc    = op->ensemble.extsrc.p;
  t.bvalues   = op->ensemble.bvalues.p;
  t.bflux     = op->ensemble.bflux.p;
  t.blk_max   = op->ensemble.blk_max.p;
  t.blk_pos   = op->ensemble.blk_pos.p;
  t.f         = f;
  t.u_out     = u_out;
  t.u_stride  = 3 * (int64_t)op->n_cells;
  t.k_stride  = 3 * (int64_t)op->K;
  t.n_members = op->ensemble.members;
  t.per_group = op->ensemble.per_group;
  t.n_buckets = ENSEMBLE_WAVES * op->grid;
  for (int m = 0; m < op->ensemble.members; ++m) t.dts[m] = dts[m];
  EnsembleKernelFn kfn = ensemble_kernel_fn(op->ensemble.hr, op->S, op->config.source_method, u_out != nullptr);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(op->grid, op->ensemble.groups), dim3(BLOCK), 0, st, a, t, u);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

// rdyhip_ensemble_enable (hr == false) / rdyhip_ens_hr_enable (hr == true): the checks, every one before any device call, then
// the allocations, the copies of the operator's inputs and the group rule -- the same for both
static int ensemble_enable(RDyHipOperator op, int32_t num_members, bool hr) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->ensemble.members != 0) return fail(RDYHIP_ERR_USER, "the ensemble is already enabled (%d members)", op->ensemble.members);
  if (num_members < 1 || num_members > RDYHIP_MAX_ENSEMBLE_MEMBERS)
    return fail(RDYHIP_ERR_USER, "num_members (%d) must be in 1..%d", num_members, RDYHIP_MAX_ENSEMBLE_MEMBERS);
  if (op->muscl || op->config.second_order) return fail(RDYHIP_ERR_USER, "ensembles are first order only (the operator was created with second_order)");
  const bool op_hr = op->hr || op->config.well_balancing != RDYHIP_WELL_BALANCING_NONE;
  if (!hr && op_hr)
    return fail(RDYHIP_ERR_USER, "ensembles with well balancing are not supported (well_balancing = %d) by rdyhip_ensemble_enable: use rdyhip_ens_hr_enable",
                op->config.well_balancing);
  if (hr && !(op->hr && op->config.well_balancing == RDYHIP_WELL_BALANCING_HR))
    return fail(RDYHIP_ERR_USER, "rdyhip_ens_hr_enable needs an operator created with RDYHIP_WELL_BALANCING_HR (well_balancing = %d): use rdyhip_ensemble_enable",
                op->config.well_balancing);
  const size_t B = (size_t)num_members, K = (size_t)op->K, no = (size_t)op->n_owned, W = (size_t)ENSEMBLE_WAVES * (size_t)op->grid;
  EnsembleState s;
  int rc = s.mannings.alloc(B * no);
  if (!rc) rc = s.extsrc.alloc(B * 3 * no);
  if (!rc) rc = s.bvalues.alloc(B * 3 * K);
  if (!rc) rc = s.bflux.zeros(B * 3 * K);
  if (!rc) rc = s.blk_max.zeros(B * W);
  if (!rc) rc = s.blk_pos.zeros(B * W);
  if (!rc) rc = s.d_courant.zeros(B);
  if (rc) return rc;
  // every member starts with the operator's own Manning's n, source and boundary values (an evaluation in flight may not
  // write them, but a stream-ordered setter may: wait for it)
  hipError_t e = hipDeviceSynchronize();
  for (size_t m = 0; m < B && e == hipSuccess; ++m) {
    if (no) e = hipMemcpy(s.mannings.p + m * no, op->d_mannings.p, sizeof(double) * no, hipMemcpyDeviceToDevice);
    if (no && e == hipSuccess) e = hipMemcpy(s.extsrc.p + m * 3 * no, op->d_extsrc.p, sizeof(double) * 3 * no, hipMemcpyDeviceToDevice);
    if (K && e == hipSuccess) e = hipMemcpy(s.bvalues.p + m * 3 * K, op->d_bvalues.p, sizeof(double) * 3 * K, hipMemcpyDeviceToDevice);
  }
  if (e == hipSuccess && B * W > 0) {
    hipLaunchKernelGGL(courant_reset_kernel, dim3(4), dim3(1024), 0, 0, (int)(B * W), s.blk_max.p, s.blk_pos.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(RDYHIP_ERR_LIB, "%s: a device copy failed: %s", hr ? "rdyhip_ens_hr_enable" : "rdyhip_ensemble_enable", hipGetErrorString(e));
  // The member groups.  Few cells: one group per member, down to ENSEMBLE_MIN_WORKGROUPS workgroups in all, so that a small
  // mesh still puts several workgroups on every CU; many cells: every thread walks up to ENSEMBLE_MAX_PER_GROUP members with
  // its geometry.
  const int64_t want = (ENSEMBLE_MIN_WORKGROUPS + (int64_t)std::max(op->grid, 1) - 1) / std::max(op->grid, 1);
  const int32_t g0   = (int32_t)std::min<int64_t>(num_members, std::max<int64_t>(want, 1));
  s.per_group  = std::min((num_members + g0 - 1) / g0, ENSEMBLE_MAX_PER_GROUP);
  s.groups     = (num_members + s.per_group - 1) / s.per_group;   // no group is empty
  s.members    = num_members;
  s.hr         = hr;
  s.courant.assign(B, RDyHipCourant{0.0, -1, -1});
  op->ensemble = std::move(s);
  return 0;
}

extern "C" int rdyhip_ensemble_enable(RDyHipOperator op, int32_t num_members) { return ensemble_enable(op, num_members, false); }

extern "C" int rdyhip_ens_hr_enable(RDyHipOperator op, int32_t num_members) { return ensemble_enable(op, num_members, true); }

extern "C" int rdyhip_ens_hr_info(RDyHipOperator op, int32_t *well_balancing) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (well_balancing) *well_balancing = op->ensemble.members != 0 && op->ensemble.hr ? RDYHIP_WELL_BALANCING_HR : RDYHIP_WELL_BALANCING_NONE;
  return 0;
}

extern "C" int rdyhip_ensemble_info(RDyHipOperator op, int32_t *num_members) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (num_members) *num_members = op->ensemble.members;
  return 0;
}

extern "C" int rdyhip_ensemble_set_mannings(RDyHipOperator op, int32_t member, int32_t n, const int32_t *owned_cell_ids, const double *values) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  if (n > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  return scatter_component(op, op->ensemble.mannings.p + (size_t)member * (size_t)op->n_owned, 1, 0, n, owned_cell_ids, values);
}

extern "C" int rdyhip_ensemble_set_external_source(RDyHipOperator op, int32_t member, int32_t comp, int32_t n, const int32_t *owned_cell_ids,
                                                   const double *values) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  if (comp < 0 || comp > 2) return fail(RDYHIP_ERR_USER, "bad source component %d", comp);
  if (n > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  return scatter_component(op, op->ensemble.extsrc.p + (size_t)member * 3 * (size_t)op->n_owned, 3, comp, n, owned_cell_ids, values);
}

extern "C" int rdyhip_ensemble_set_boundary_values(RDyHipOperator op, int32_t member, int32_t boundary, int32_t num_edges, const double *values) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  return boundary_rows_copy(op, boundary, num_edges, op->ensemble.bvalues.p + 3 * (size_t)member * (size_t)op->K, 3, const_cast<double *>(values), true);
}

extern "C" int rdyhip_ensemble_rhs_function(RDyHipOperator op, const double *dts, const double *u_local, double *f_global, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!dts) return fail(RDYHIP_ERR_USER, "null dts");
  if (op->n_owned > 0 && (!u_local || !f_global)) return fail(RDYHIP_ERR_USER, "null u_local / f_global");
  return launch_ensemble(op, dts, u_local, f_global, nullptr, (hipStream_t)stream);
}

extern "C" int rdyhip_ensemble_euler_step(RDyHipOperator op, const double *dts, const double *u_local, double *u_local_out, double *f_global, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!dts) return fail(RDYHIP_ERR_USER, "null dts");
  if (op->n_owned > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  rc = euler_out_check(op, "rdyhip_ensemble_euler_step", u_local, u_local_out);
  if (rc) return rc;
  return launch_ensemble(op, dts, u_local, f_global, u_local_out, (hipStream_t)stream);
}

extern "C" int rdyhip_ensemble_get_boundary_fluxes(RDyHipOperator op, int32_t member, int32_t boundary, int32_t num_edges, double *fluxes) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  return boundary_rows_copy(op, boundary, num_edges, op->ensemble.bflux.p + 3 * (size_t)member * (size_t)op->K, 3, fluxes, false);
}

extern "C" int rdyhip_ensemble_update_diagnostics(RDyHipOperator op, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  rc = diagnostics_read_discard(op->diag_read[RDYHIP_DIAGNOSTICS_ENSEMBLE], (hipStream_t)stream);
  if (rc) return rc;
  const int B = op->ensemble.members;
  hipLaunchKernelGGL(ensemble_courant_finalize_kernel, dim3(B), dim3(BLOCK), 0, (hipStream_t)stream, ENSEMBLE_WAVES * op->grid, op->ensemble.blk_max.p,
                     op->ensemble.blk_pos.p, op->ensemble.d_courant.p);
  HIP_TRY(hipGetLastError());
  DeviceCourant dc[RDYHIP_MAX_ENSEMBLE_MEMBERS];
  HIP_TRY(hipMemcpyAsync(dc, op->ensemble.d_courant.p, sizeof(DeviceCourant) * (size_t)B, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  for (int m = 0; m < B; ++m) op->ensemble.courant[m] = courant_from_device(op, dc[m], true);
  return 0;
}

extern "C" int rdyhip_ensemble_get_diagnostics(RDyHipOperator op, RDyHipCourant *courant) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!courant) return fail(RDYHIP_ERR_USER, "null argument");
  for (int m = 0; m < op->ensemble.members; ++m) courant[m] = op->ensemble.courant[m];
  return 0;
}
