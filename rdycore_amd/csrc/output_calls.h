// Time-averaged output fields behind the C ABI (rdyhip_output_mean_*; kernels: output_kernels.h): the accumulators of the
// solution, the primitive variables and the sources, and their means.  Included by rdyhip_api.hip only, after
// output_shared.h (the checks, enable, get, reset and time that the tracer and ensemble means share).
#pragma once
namespace {

// null operator, unknown bits, not exactly one variable: the argument errors the five calls share
int output_check(RDyHipOperator op, int32_t vars, bool single) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  return means_check_vars(vars, single);
}

}  // namespace

extern "C" int rdyhip_output_mean_enable(RDyHipOperator op, int32_t vars) {
  int rc = output_check(op, vars, false);
  if (rc) return rc;
  return means_enable(op->means, vars, (size_t)3 * op->n_owned, 1);
}

extern "C" int rdyhip_output_mean_accumulate(RDyHipOperator op, int32_t vars, double dt, const double *u_local, void *stream) {
  int rc = output_check(op, vars, false);
  if (!rc) rc = means_check_enabled(op->means, SWE_WORDS, vars);
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
                       op->n_owned, owned_to_local(op), dt, us, acc_s, u_prev, pv_stored, tiny_h, ha2, acc_p, ext, acc_x);
    HIP_TRY(hipGetLastError());
  }
  for (int i = 0; i < 3; ++i)
    if (vars >> i & 1) op->means.time[i][0] += dt;   // AccumulateOutputVar: accumulated_time += dt
  return 0;
}

extern "C" int rdyhip_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean, double *accumulated_time, void *stream) {
  int rc = output_check(op, var, true);
  if (!rc) rc = means_check_enabled(op->means, SWE_WORDS, var);
  if (rc) return rc;
  return means_get(op, op->means, SWE_WORDS, var, 3, d_mean, accumulated_time, (hipStream_t)stream);
}

extern "C" int rdyhip_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream) {
  int rc = output_check(op, vars, false);
  if (!rc) rc = means_check_enabled(op->means, SWE_WORDS, vars);
  if (rc) return rc;
  return means_reset(op, op->means, vars, (hipStream_t)stream);
}

extern "C" int rdyhip_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_time) {
  int rc = output_check(op, var, true);
  if (rc) return rc;
  if (!accumulated_time) return fail(RDYHIP_ERR_USER, "null accumulated_time");
  return means_time(op->means, SWE_WORDS, var, accumulated_time);
}
