// The non-blocking read-back of the Courant record(s) behind the C ABI (rdyhip_diagnostics_begin / _ready / _wait): the merge
// launch of the blocking calls (courant_finalize_kernel, ensemble_courant_finalize_kernel: swe_kernels.h, ensemble_kernels.h),
// a copy into pinned memory and an event, all on the caller's stream; the host waits on that event alone.  Included by
// rdyhip_api.hip only.
#pragma once
namespace {

// null operator, unknown scope, ensemble scope before rdyhip_ensemble_enable: before any device call
int diagnostics_check(RDyHipOperator op, int32_t scope) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (scope != RDYHIP_DIAGNOSTICS_OPERATOR && scope != RDYHIP_DIAGNOSTICS_ENSEMBLE)
    return fail(RDYHIP_ERR_USER, "unknown diagnostics scope %d (RDYHIP_DIAGNOSTICS_*)", scope);
  if (scope == RDYHIP_DIAGNOSTICS_ENSEMBLE && op->ensemble.members == 0)
    return fail(RDYHIP_ERR_USER, "the ensemble is not enabled (rdyhip_ensemble_enable)");
  return 0;
}

int diagnostics_nothing_begun(int32_t scope) {
  return fail(RDYHIP_ERR_USER, "no diagnostics read of scope %d is in flight (rdyhip_diagnostics_begin)", scope);
}

}  // namespace

extern "C" int rdyhip_diagnostics_begin(RDyHipOperator op, int32_t scope, void *stream) {
  int rc = diagnostics_check(op, scope);
  if (rc) return rc;
  DiagnosticsRead &r  = op->diag_read[scope];
  hipStream_t      st = (hipStream_t)stream;
  const bool       ens = scope == RDYHIP_DIAGNOSTICS_ENSEMBLE;
  // the first begin of the scope allocates (and may synchronise)
  if (!r.h_rec) HIP_TRY(hipHostMalloc((void **)&r.h_rec, sizeof(DeviceCourant) * (ens ? RDYHIP_MAX_ENSEMBLE_MEMBERS : 1), hipHostMallocDefault));
  if (!r.done) HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  // an earlier read that was not waited for is replaced; its copy may still be reading the device record, on any stream
  rc = diagnostics_read_discard(r, st);
  if (rc) return rc;
  r.state = DiagnosticsRead::NONE;
  if (ens) {
    const int B = op->ensemble.members;
    hipLaunchKernelGGL(ensemble_courant_finalize_kernel, dim3(B), dim3(BLOCK), 0, st, ENSEMBLE_WAVES * op->grid, op->ensemble.blk_max.p,
                       op->ensemble.blk_pos.p, op->ensemble.d_courant.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(r.h_rec, op->ensemble.d_courant.p, sizeof(DeviceCourant) * (size_t)B, hipMemcpyDeviceToHost, st));
  } else {
    hipLaunchKernelGGL(courant_finalize_kernel, dim3(1), dim3(1024), 0, st, (int)op->d_blk_max.n, op->d_blk_max.p, op->d_blk_pos.p, op->d_courant.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(r.h_rec, op->d_courant.p, sizeof(DeviceCourant), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipEventRecord(r.done, st));
  r.owned_side = ens || op->courant_owned_side;   // a later evaluation of the other kind may flip the operator's flag
  r.state      = DiagnosticsRead::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_diagnostics_ready(RDyHipOperator op, int32_t scope, int32_t *ready) {
  int rc = diagnostics_check(op, scope);
  if (rc) return rc;
  if (!ready) return fail(RDYHIP_ERR_USER, "null argument");
  const DiagnosticsRead &r = op->diag_read[scope];
  if (r.state == DiagnosticsRead::NONE) return diagnostics_nothing_begun(scope);
  *ready = 1;
  if (r.state == DiagnosticsRead::IN_FLIGHT) {
    const hipError_t e = hipEventQuery(r.done);
    if (e == hipErrorNotReady) {
      (void)hipGetLastError();
      *ready = 0;
    } else {
      HIP_TRY(e);
    }
  }
  return 0;
}

extern "C" int rdyhip_diagnostics_wait(RDyHipOperator op, int32_t scope) {
  int rc = diagnostics_check(op, scope);
  if (rc) return rc;
  DiagnosticsRead &r = op->diag_read[scope];
  if (r.state != DiagnosticsRead::IN_FLIGHT) return diagnostics_nothing_begun(scope);
  HIP_TRY(hipEventSynchronize(r.done));
  r.state = DiagnosticsRead::LANDED;
  if (scope == RDYHIP_DIAGNOSTICS_ENSEMBLE) {
    for (int m = 0; m < op->ensemble.members; ++m) op->ensemble.courant[m] = courant_from_device(op, r.h_rec[m], true);
  } else {
    op->courant = courant_from_device(op, r.h_rec[0], r.owned_side);
  }
  return 0;
}
