// Time-averaged output fields behind the C ABI (rdyhip_output_mean_*; kernels: output_kernels.h): the accumulators of the
// solution, the primitive variables and the sources, and their means.  Included by rdyhip_api.hip only, after rk_calls.h
// (aligned16).
#pragma once
namespace {

constexpr int32_t OUT_VARS = RDYHIP_OUTPUT_SOLUTION | RDYHIP_OUTPUT_PRIMITIVE_VARIABLES | RDYHIP_OUTPUT_SOURCES;

// null operator, unknown bits, a variable without an accumulator: the argument errors the five calls share
int output_check(RDyHipOperator op, int32_t vars, bool single) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (vars & ~OUT_VARS) return fail(RDYHIP_ERR_USER, "unknown output variable bits 0x%x", (unsigned)(vars & ~OUT_VARS));
  if (single && vars != RDYHIP_OUTPUT_SOLUTION && vars != RDYHIP_OUTPUT_PRIMITIVE_VARIABLES && vars != RDYHIP_OUTPUT_SOURCES)
    return fail(RDYHIP_ERR_USER, "exactly one output variable is needed (got 0x%x)", (unsigned)vars);
  return 0;
}
int output_check_enabled(RDyHipOperator op, int32_t vars) {
  for (int i = 0; i < 3; ++i)
    if ((vars >> i & 1) && !op->means.acc[i].p)
      return fail(RDYHIP_ERR_USER, "output variable 0x%x is not enabled (rdyhip_output_mean_enable)", 1u << i);
  return 0;
}
int output_index(int32_t var) { return var == RDYHIP_OUTPUT_SOLUTION ? 0 : var == RDYHIP_OUTPUT_PRIMITIVE_VARIABLES ? 1 : 2; }

}  // namespace

extern "C" int rdyhip_output_mean_enable(RDyHipOperator op, int32_t vars) {
  int rc = output_check(op, vars, false);
  if (rc) return rc;
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1) || op->means.acc[i].p) continue;   // an existing accumulator keeps its content
    DevBuf<double> a;
    rc = a.zeros((size_t)3 * op->n_owned);
    if (rc) return rc;
    op->means.acc[i]  = std::move(a);
    op->means.time[i] = 0.0;
  }
  return 0;
}

extern "C" int rdyhip_output_mean_accumulate(RDyHipOperator op, int32_t vars, double dt, const double *u_local, void *stream) {
  int rc = output_check(op, vars, false);
  if (!rc) rc = output_check_enabled(op, vars);
  if (rc) return rc;
  const bool sol = vars & RDYHIP_OUTPUT_SOLUTION, prim = vars & RDYHIP_OUTPUT_PRIMITIVE_VARIABLES, src = vars & RDYHIP_OUTPUT_SOURCES;
  if (sol && op->n_owned > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local (needed with RDYHIP_OUTPUT_SOLUTION)");
  if (op->n_owned > 0 && vars) {
    // The primitive variables of the most recent evaluation: the stored array while the evaluations store (or none has run
    // since the last store: the zeros of create included), else formed from that evaluation's state, which is the caller's
    // array -- checked as pv_hand_out checks it.  pv_wanted / pv_pending and the modes of the source are left as they are.
    // (After a pv_hand_out that failed on its own check, pv_wanted is on with d_pv not brought up to date: the stored rows are
    // then the last storing evaluation's until the next evaluation writes them -- rdyhip.h says so -- and are summed as such.)
    const double *u_prev = nullptr, *pv_stored = nullptr;
    if (prim) {
      if (op->pv_wanted || !op->pv_pending) {
        pv_stored = op->d_pv.p;
      } else {
        u_prev = op->pv_u;
        hipPointerAttribute_t at{};
        const hipError_t      e = u_prev ? hipPointerGetAttributes(&at, u_prev) : hipErrorInvalidValue;
        if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != op->device) {
          (void)hipGetLastError();
          return fail(RDYHIP_ERR_USER, "output means: the state array of the last evaluation is gone (not device memory of device %d any more)",
                      op->device);
        }
      }
    }
    const double *us = sol ? u_local : nullptr, *ext = src ? op->d_extsrc.p : nullptr;
    double       *acc_s = sol ? op->means.acc[0].p : nullptr, *acc_p = prim ? op->means.acc[1].p : nullptr, *acc_x = src ? op->means.acc[2].p : nullptr;
    const double  tiny_h = op->config.tiny_h, ha2 = op->config.h_anuga_regular * op->config.h_anuga_regular;
    hipLaunchKernelGGL(output_accumulate_kernel, dim3((unsigned)((op->n_owned + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, (hipStream_t)stream,
                       op->n_owned, op->prefix ? (const int32_t *)nullptr : op->d_o2l.p, dt, us, acc_s, u_prev, pv_stored, tiny_h, ha2, acc_p, ext, acc_x);
    HIP_TRY(hipGetLastError());
  }
  for (int i = 0; i < 3; ++i)
    if (vars >> i & 1) op->means.time[i] += dt;   // AccumulateOutputVar: accumulated_time += dt
  return 0;
}

extern "C" int rdyhip_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean, double *accumulated_time, void *stream) {
  int rc = output_check(op, var, true);
  if (!rc) rc = output_check_enabled(op, var);
  if (rc) return rc;
  const int i = output_index(var);
  if (op->n_owned > 0 && !d_mean) return fail(RDYHIP_ERR_USER, "null d_mean");
  // ComputeMean's PetscCheck (src/xdmf_output.c:213)
  if (!(op->means.time[i] > 0.0)) return fail(RDYHIP_ERR_USER, "output variable 0x%x: no time has been accumulated", (unsigned)var);
  if (accumulated_time) *accumulated_time = op->means.time[i];
  const int64_t n = 3 * (int64_t)op->n_owned;
  if (n == 0) return 0;
  const double  s   = 1.0 / op->means.time[i];
  const double *acc = op->means.acc[i].p;
  if (aligned16(acc) && aligned16(d_mean)) {
    const int64_t pairs = (n + 1) / 2;
    hipLaunchKernelGGL((output_mean_kernel<true>), dim3((unsigned)((pairs + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, (hipStream_t)stream, n, s,
                       acc, d_mean);
  } else {
    hipLaunchKernelGGL((output_mean_kernel<false>), dim3((unsigned)((n + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, (hipStream_t)stream, n, s, acc,
                       d_mean);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int rdyhip_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream) {
  int rc = output_check(op, vars, false);
  if (!rc) rc = output_check_enabled(op, vars);
  if (rc) return rc;
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1)) continue;
    if (op->n_owned > 0) HIP_TRY(hipMemsetAsync(op->means.acc[i].p, 0, op->means.acc[i].bytes(), (hipStream_t)stream));
    op->means.time[i] = 0.0;
  }
  return 0;
}

extern "C" int rdyhip_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_time) {
  int rc = output_check(op, var, true);
  if (rc) return rc;
  if (!accumulated_time) return fail(RDYHIP_ERR_USER, "null accumulated_time");
  rc = output_check_enabled(op, var);
  if (rc) return rc;
  *accumulated_time = op->means.time[output_index(var)];
  return 0;
}

