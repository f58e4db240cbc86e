// Output of the tracer state behind the C ABI (rdyhip_tracer_state_*, rdyhip_tracer_error_sums*, rdyhip_tracer_output_mean_*,
// rdyhip_tracer_series_*; kernels: tracer_output_kernels.h): the read-out, error sums, output means and observation series of
// readout_calls.h, output_calls.h and series_calls.h for rows of N = 3 + NT.  Included by rdyhip_api.hip only, after
// tracer_calls.h (tracers_check) and those three (sums_reserve, OUT_VARS, output_index, aligned16).
#pragma once
namespace {

// f(std::integral_constant<int, NT>) for the operator's number of tracers: how a launch picks its instantiation
template <class F>
int with_tracer_count(int nt, F f) {
  switch (nt) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    default: return f(std::integral_constant<int, 7>());
  }
}

int tout_width(RDyHipOperator op) { return 3 + op->tracers.n; }
int tout_popcount(int32_t comps) { return __builtin_popcount((unsigned)comps); }

// null operator, tracers not enabled, then the mask: bits 0 .. N - 1, at least one (single: exactly one)
int tout_check_comps(RDyHipOperator op, int32_t comps, bool single) {
  int rc = tracers_check(op);
  if (rc) return rc;
  const int N = tout_width(op);
  if (comps < 1 || comps >= (1 << N))
    return fail(RDYHIP_ERR_USER, "component mask 0x%x is not in 1..0x%x (bit i: component i of the %d of a row)", (unsigned)comps, (1u << N) - 1, N);
  if (single && (comps & (comps - 1))) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comps);
  return 0;
}
int tout_check_form(int32_t form) {
  if (form != RDYHIP_TRACER_FORM_CONSERVED && form != RDYHIP_TRACER_FORM_PRIMITIVE)
    return fail(RDYHIP_ERR_USER, "unknown form %d (RDYHIP_TRACER_FORM_CONSERVED, RDYHIP_TRACER_FORM_PRIMITIVE)", form);
  return 0;
}

int launch_tracer_planes(RDyHipOperator op, int32_t comps, int32_t form, const double *u, double *planes, hipStream_t st) {
  const dim3     grid((unsigned)((op->n_owned + TOUT_BLOCK - 1) / TOUT_BLOCK));
  const int32_t *o2l = op->prefix ? (const int32_t *)nullptr : op->d_o2l.p;
  const double   tiny_h = op->config.tiny_h, ha2 = op->config.h_anuga_regular * op->config.h_anuga_regular;
  return with_tracer_count(op->tracers.n, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    if (form == RDYHIP_TRACER_FORM_PRIMITIVE)
      hipLaunchKernelGGL((tracer_planes_kernel<NT, true>), grid, dim3(TOUT_BLOCK), 0, st, op->n_owned, o2l, (int)comps, tiny_h, ha2, (const uint64_t *)u,
                         (uint64_t *)planes);
    else
      hipLaunchKernelGGL((tracer_planes_kernel<NT, false>), grid, dim3(TOUT_BLOCK), 0, st, op->n_owned, o2l, (int)comps, tiny_h, ha2, (const uint64_t *)u,
                         (uint64_t *)planes);
    HIP_TRY(hipGetLastError());
    return 0;
  });
}

// read_reserve (readout_calls.h) for the tracer read-out's own buffers and events; the copy stream is the operator's
int tout_read_reserve(RDyHipOperator op, int k) {
  TracerOutput &r = op->tracer_out;
  if (!op->stage.copy) HIP_TRY(hipStreamCreateWithFlags(&op->stage.copy, hipStreamNonBlocking));
  if (!r.launched) HIP_TRY(hipEventCreateWithFlags(&r.launched, hipEventDisableTiming));
  if (!r.done) HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  const size_t need = (size_t)k * (size_t)op->n_owned;
  if (r.d_planes.p && r.d_planes.n >= need && r.h_cap >= need) return 0;
  if (r.state == TracerOutput::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.done));
  r.state = TracerOutput::NONE;   // whatever had been read lived in the old buffers
  int rc = r.d_planes.alloc(need);
  if (rc) return rc;
  if (r.h_planes) HIP_TRY(hipHostFree(r.h_planes));
  r.h_planes = nullptr;
  r.h_cap    = 0;
  HIP_TRY(hipHostMalloc((void **)&r.h_planes, sizeof(double) * need, hipHostMallocDefault));
  r.h_cap = need;
  return 0;
}

// the state checks of _get and _ptr; *plane = the index of `comp` among the planes of the last begin
int tout_check_landed(RDyHipOperator op, int32_t comp, int *plane) {
  const TracerOutput &r = op->tracer_out;
  if (r.state != TracerOutput::LANDED)
    return fail(RDYHIP_ERR_USER, r.state == TracerOutput::NONE ? "no tracer state read has been begun (rdyhip_tracer_state_read_begin)"
                                                               : "the tracer state read has not been waited for (rdyhip_tracer_state_read_wait)");
  if (!(r.comps & comp))
    return fail(RDYHIP_ERR_USER, "component 0x%x was not asked for by the last rdyhip_tracer_state_read_begin (0x%x)", (unsigned)comp, (unsigned)r.comps);
  *plane = tout_popcount(r.comps & (comp - 1));
  return 0;
}

// the shared area table (and the workgroup count that goes with n_owned), this feature's records and pinned result
int tout_sums_reserve(RDyHipOperator op) {
  int rc = sums_reserve(op);
  if (rc) return rc;
  TracerOutput &r = op->tracer_out;
  const size_t  V = 3 * (size_t)tout_width(op) + 1;
  if (!r.sums_done) HIP_TRY(hipEventCreateWithFlags(&r.sums_done, hipEventDisableTiming));
  if (!r.h_sums) HIP_TRY(hipHostMalloc((void **)&r.h_sums, sizeof(double) * V, hipHostMallocDefault));
  if (!r.d_records.p) {
    DevBuf<double> records;
    rc = records.alloc((size_t)(op->readout.err_wg + 1) * V);
    if (rc) return rc;
    r.d_records = std::move(records);
  }
  return 0;
}

// null operator, tracers not enabled, unknown bits, not exactly one variable: the argument errors the five mean calls share
int tout_means_check(RDyHipOperator op, int32_t vars, bool single) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (vars & ~OUT_VARS) return fail(RDYHIP_ERR_USER, "unknown output variable bits 0x%x", (unsigned)(vars & ~OUT_VARS));
  if (single && vars != RDYHIP_OUTPUT_SOLUTION && vars != RDYHIP_OUTPUT_PRIMITIVE_VARIABLES && vars != RDYHIP_OUTPUT_SOURCES)
    return fail(RDYHIP_ERR_USER, "exactly one output variable is needed (got 0x%x)", (unsigned)vars);
  return 0;
}
int tout_means_check_enabled(RDyHipOperator op, int32_t vars) {
  for (int i = 0; i < 3; ++i)
    if ((vars >> i & 1) && !op->tracer_out.acc[i].p)
      return fail(RDYHIP_ERR_USER, "tracer output variable 0x%x is not enabled (rdyhip_tracer_output_mean_enable)", 1u << i);
  return 0;
}

int tout_series_check(RDyHipOperator op) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!op->tracer_out.series_enabled) return fail(RDYHIP_ERR_USER, "the tracer observation series is not enabled (rdyhip_tracer_series_enable)");
  return 0;
}

}  // namespace

extern "C" int rdyhip_tracer_state_planes(RDyHipOperator op, int32_t comps, int32_t form, const double *u_local, double *d_planes, void *stream) {
  int rc = tout_check_comps(op, comps, false);
  if (!rc) rc = tout_check_form(form);
  if (rc) return rc;
  if (op->n_owned == 0) return 0;
  if (!u_local || !d_planes) return fail(RDYHIP_ERR_USER, "null u_local / d_planes");
  return launch_tracer_planes(op, comps, form, u_local, d_planes, (hipStream_t)stream);
}

extern "C" int rdyhip_tracer_state_read_begin(RDyHipOperator op, int32_t comps, int32_t form, const double *u_local, void *stream) {
  int rc = tout_check_comps(op, comps, false);
  if (!rc) rc = tout_check_form(form);
  if (rc) return rc;
  TracerOutput &r = op->tracer_out;
  if (op->n_owned == 0) {   // nothing is launched or copied: the read has landed as soon as it is waited for
    r.comps = comps;
    r.state = TracerOutput::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  hipStream_t st = (hipStream_t)stream;
  const int   k  = tout_popcount(comps);
  rc = tout_read_reserve(op, k);
  if (rc) return rc;
  // an earlier read that has not landed is given up; its copy may still be reading the device planes, so this launch waits for it
  if (r.state == TracerOutput::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.done, 0));
  r.state = TracerOutput::NONE;
  rc = launch_tracer_planes(op, comps, form, u_local, r.d_planes.p, st);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(r.launched, st));
  HIP_TRY(hipStreamWaitEvent(op->stage.copy, r.launched, 0));
  HIP_TRY(hipMemcpyAsync(r.h_planes, r.d_planes.p, sizeof(double) * (size_t)k * (size_t)op->n_owned, hipMemcpyDeviceToHost, op->stage.copy));
  HIP_TRY(hipEventRecord(r.done, op->stage.copy));
  r.comps = comps;
  r.state = TracerOutput::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_tracer_state_read_ready(RDyHipOperator op, int32_t *ready) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!ready) return fail(RDYHIP_ERR_USER, "null argument");
  const TracerOutput &r = op->tracer_out;
  if (r.state == TracerOutput::NONE) return fail(RDYHIP_ERR_USER, "no tracer state read has been begun (rdyhip_tracer_state_read_begin)");
  *ready = 1;
  if (r.state == TracerOutput::IN_FLIGHT && op->n_owned > 0) {
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

extern "C" int rdyhip_tracer_state_read_wait(RDyHipOperator op) {
  int rc = tracers_check(op);
  if (rc) return rc;
  TracerOutput &r = op->tracer_out;
  if (r.state == TracerOutput::NONE) return fail(RDYHIP_ERR_USER, "no tracer state read has been begun (rdyhip_tracer_state_read_begin)");
  if (r.state == TracerOutput::IN_FLIGHT && op->n_owned > 0) HIP_TRY(hipEventSynchronize(r.done));
  r.state = TracerOutput::LANDED;
  return 0;
}

extern "C" int rdyhip_tracer_state_read_get(RDyHipOperator op, int32_t comp, int32_t size, double *values) {
  int rc = tout_check_comps(op, comp, true);
  if (rc) return rc;
  // CheckNumOwnedCells (src/rdydata.c:54-58)
  if (size != op->n_owned) return fail(RDYHIP_ERR_ARG_SIZ, "The size of array (%d) is not equal to the number of owned cells (%d)", size, op->n_owned);
  if (size > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  int plane = 0;
  rc = tout_check_landed(op, comp, &plane);
  if (rc) return rc;
  if (size > 0) memcpy(values, op->tracer_out.h_planes + (size_t)plane * (size_t)op->n_owned, sizeof(double) * (size_t)size);
  return 0;
}

extern "C" int rdyhip_tracer_state_read_ptr(RDyHipOperator op, int32_t comp, const double **pinned_values) {
  int rc = tout_check_comps(op, comp, true);
  if (rc) return rc;
  if (!pinned_values) return fail(RDYHIP_ERR_USER, "null argument");
  int plane = 0;
  rc = tout_check_landed(op, comp, &plane);
  if (rc) return rc;
  *pinned_values = op->n_owned > 0 ? op->tracer_out.h_planes + (size_t)plane * (size_t)op->n_owned : nullptr;
  return 0;
}

extern "C" int rdyhip_tracer_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream) {
  int rc = tracers_check(op);
  if (rc) return rc;
  TracerOutput &r = op->tracer_out;
  if (op->n_owned == 0) {   // all zeros, nothing launched
    r.sums_state = TracerOutput::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  rc = tout_sums_reserve(op);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the records and the pinned result are shared by all calls: this one is ordered behind an earlier one that is still running
  if (r.sums_state == TracerOutput::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.sums_done, 0));
  const int      wg = op->readout.err_wg;
  const size_t   V  = 3 * (size_t)tout_width(op) + 1;
  double        *result = r.d_records.p + (size_t)wg * V;
  const int32_t *o2l = op->prefix ? (const int32_t *)nullptr : op->d_o2l.p;
  rc = with_tracer_count(op->tracers.n, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    hipLaunchKernelGGL((tracer_error_partial_kernel<NT>), dim3(wg), dim3(ERR_BLOCK), 0, st, op->n_owned, o2l, u_local, d_exact, op->readout.d_area.p,
                       r.d_records.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((tracer_error_finalize_kernel<NT>), dim3(1), dim3(ERR_BLOCK), 0, st, wg, r.d_records.p, result);
    HIP_TRY(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(r.h_sums, result, sizeof(double) * V, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(r.sums_done, st));
  r.sums_state = TracerOutput::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_tracer_error_sums_get(RDyHipOperator op, RDyHipTracerErrorSums *out) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!out) return fail(RDYHIP_ERR_USER, "null argument");
  TracerOutput &r = op->tracer_out;
  if (r.sums_state == TracerOutput::NONE) return fail(RDYHIP_ERR_USER, "no tracer error sums have been asked for (rdyhip_tracer_error_sums)");
  static_assert(sizeof(RDyHipTracerErrorSums) == sizeof(double) * (3 * (3 + RDYHIP_MAX_TRACERS) + 1), "three arrays of the widest row and the area");
  memset(out, 0, sizeof(*out));   // entries >= N stay 0
  if (op->n_owned > 0) {
    if (r.sums_state == TracerOutput::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.sums_done));
    const int N = tout_width(op);
    for (int c = 0; c < N; ++c) {
      out->l1[c]         = r.h_sums[c];
      out->l2_squared[c] = r.h_sums[N + c];
      out->linf[c]       = r.h_sums[2 * N + c];
    }
    out->area = r.h_sums[3 * N];
  }
  r.sums_state = TracerOutput::LANDED;
  return 0;
}

extern "C" int rdyhip_tracer_output_mean_enable(RDyHipOperator op, int32_t vars) {
  int rc = tout_means_check(op, vars, false);
  if (rc) return rc;
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1) || op->tracer_out.acc[i].p) continue;   // an existing accumulator keeps its content
    DevBuf<double> a;
    rc = a.zeros((size_t)tout_width(op) * op->n_owned);
    if (rc) return rc;
    op->tracer_out.acc[i]  = std::move(a);
    op->tracer_out.time[i] = 0.0;
  }
  return 0;
}

extern "C" int rdyhip_tracer_output_mean_accumulate(RDyHipOperator op, int32_t vars, double dt, const double *u_solution, const double *u_primitive,
                                                    void *stream) {
  int rc = tout_means_check(op, vars, false);
  if (!rc) rc = tout_means_check_enabled(op, vars);
  if (rc) return rc;
  const bool sol = vars & RDYHIP_OUTPUT_SOLUTION, prim = vars & RDYHIP_OUTPUT_PRIMITIVE_VARIABLES, src = vars & RDYHIP_OUTPUT_SOURCES;
  if (sol && op->n_owned > 0 && !u_solution) return fail(RDYHIP_ERR_USER, "null u_solution (needed with RDYHIP_OUTPUT_SOLUTION)");
  if (prim && op->n_owned > 0 && !u_primitive) return fail(RDYHIP_ERR_USER, "null u_primitive (needed with RDYHIP_OUTPUT_PRIMITIVE_VARIABLES)");
  TracerOutput &t = op->tracer_out;
  if (op->n_owned > 0 && vars) {
    // the sources: the canonical [owned][3] array, which every writer keeps current whatever the water-only and uniform modes of
    // the SWE kernels are (operator_state.h), and the tracers' [owned][NT]; both read at this place in the stream
    const double *us = sol ? u_solution : nullptr, *up = prim ? u_primitive : nullptr;
    double       *acc_s = sol ? t.acc[0].p : nullptr, *acc_p = prim ? t.acc[1].p : nullptr, *acc_x = src ? t.acc[2].p : nullptr;
    const double  tiny_h = op->config.tiny_h, ha2 = op->config.h_anuga_regular * op->config.h_anuga_regular;
    const int32_t *o2l = op->prefix ? (const int32_t *)nullptr : op->d_o2l.p;
    rc = with_tracer_count(op->tracers.n, [&](auto nt) {
      constexpr int NT = decltype(nt)::value;
      hipLaunchKernelGGL((tracer_output_accumulate_kernel<NT>), dim3((unsigned)((op->n_owned + TOUT_BLOCK - 1) / TOUT_BLOCK)), dim3(TOUT_BLOCK), 0,
                         (hipStream_t)stream, op->n_owned, o2l, dt, us, acc_s, up, tiny_h, ha2, acc_p, (const double *)op->d_extsrc.p,
                         (const double *)op->tracers.src.p, acc_x);
      HIP_TRY(hipGetLastError());
      return 0;
    });
    if (rc) return rc;
  }
  for (int i = 0; i < 3; ++i)
    if (vars >> i & 1) t.time[i] += dt;   // AccumulateOutputVar: accumulated_time += dt
  return 0;
}

extern "C" int rdyhip_tracer_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean, double *accumulated_time, void *stream) {
  int rc = tout_means_check(op, var, true);
  if (!rc) rc = tout_means_check_enabled(op, var);
  if (rc) return rc;
  const int     i = output_index(var);
  TracerOutput &t = op->tracer_out;
  if (op->n_owned > 0 && !d_mean) return fail(RDYHIP_ERR_USER, "null d_mean");
  // ComputeMean's PetscCheck (src/xdmf_output.c:213)
  if (!(t.time[i] > 0.0)) return fail(RDYHIP_ERR_USER, "tracer output variable 0x%x: no time has been accumulated", (unsigned)var);
  if (accumulated_time) *accumulated_time = t.time[i];
  const int64_t n = (int64_t)tout_width(op) * op->n_owned;
  if (n == 0) return 0;
  const double  s   = 1.0 / t.time[i];
  const double *acc = t.acc[i].p;
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

extern "C" int rdyhip_tracer_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream) {
  int rc = tout_means_check(op, vars, false);
  if (!rc) rc = tout_means_check_enabled(op, vars);
  if (rc) return rc;
  TracerOutput &t = op->tracer_out;
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1)) continue;
    if (op->n_owned > 0) HIP_TRY(hipMemsetAsync(t.acc[i].p, 0, t.acc[i].bytes(), (hipStream_t)stream));
    t.time[i] = 0.0;
  }
  return 0;
}

extern "C" int rdyhip_tracer_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_time) {
  int rc = tout_means_check(op, var, true);
  if (rc) return rc;
  if (!accumulated_time) return fail(RDYHIP_ERR_USER, "null accumulated_time");
  rc = tout_means_check_enabled(op, var);
  if (rc) return rc;
  *accumulated_time = op->tracer_out.time[output_index(var)];
  return 0;
}

extern "C" int rdyhip_tracer_series_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids, int32_t capacity) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (num_sites < 0 || capacity < 0) return fail(RDYHIP_ERR_USER, "negative number of sites (%d) or capacity (%d)", num_sites, capacity);
  if (num_sites > 0 && !owned_cell_ids) return fail(RDYHIP_ERR_USER, "null owned_cell_ids");
  TracerOutput &t = op->tracer_out;
  if (t.series_enabled) return fail(RDYHIP_ERR_USER, "the tracer observation series is enabled already");
  for (int32_t i = 0; i < num_sites; ++i)
    if (owned_cell_ids[i] < 0 || owned_cell_ids[i] >= op->n_owned)
      return fail(RDYHIP_ERR_USER, "observation site %d: owned cell %d out of range [0, %d)", i, owned_cell_ids[i], op->n_owned);
  std::vector<int32_t> local(owned_cell_ids, owned_cell_ids + num_sites);
  if (!op->prefix && num_sites > 0) {   // owned -> local through the operator's own table
    std::vector<int32_t> o2l((size_t)op->n_owned);
    HIP_TRY(hipMemcpy(o2l.data(), op->d_o2l.p, sizeof(int32_t) * (size_t)op->n_owned, hipMemcpyDeviceToHost));
    for (auto &c : local) c = o2l[(size_t)c];
  }
  DevBuf<int32_t> sites;
  DevBuf<double>  log;
  rc = sites.upload(local);
  if (!rc) rc = log.zeros((size_t)capacity * (size_t)num_sites * (size_t)tout_width(op));
  if (rc) return rc;
  t.d_sites  = std::move(sites);
  t.d_log    = std::move(log);
  t.entries  = num_sites;
  t.capacity = capacity;
  t.times.clear();
  t.times.reserve((size_t)capacity);
  t.series_enabled = true;
  return 0;
}

extern "C" int rdyhip_tracer_series_record(RDyHipOperator op, double time, const double *u_local, void *stream) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  TracerOutput &t = op->tracer_out;
  if (t.entries > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  if ((int64_t)t.times.size() >= (int64_t)t.capacity)
    return fail(RDYHIP_ERR_USER, "tracer series: the log is full (%d records); read it and call rdyhip_tracer_series_clear", t.capacity);
  const int64_t r = (int64_t)t.times.size();
  if (t.entries > 0) {
    rc = with_tracer_count(op->tracers.n, [&](auto nt) {
      constexpr int NT = decltype(nt)::value;
      hipLaunchKernelGGL((tracer_series_observe_kernel<NT>), dim3((unsigned)((t.entries + SERIES_BLOCK - 1) / SERIES_BLOCK)), dim3(SERIES_BLOCK), 0,
                         (hipStream_t)stream, t.entries, (const int32_t *)t.d_sites.p, u_local, r, t.d_log.p);
      HIP_TRY(hipGetLastError());
      return 0;
    });
    if (rc) return rc;
  }
  t.times.push_back(time);
  return 0;
}

extern "C" int rdyhip_tracer_series_info(RDyHipOperator op, int32_t *entries, int32_t *count, int32_t *capacity) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  const TracerOutput &t = op->tracer_out;
  if (entries) *entries = t.entries;
  if (count) *count = (int32_t)t.times.size();
  if (capacity) *capacity = t.capacity;
  return 0;
}

extern "C" int rdyhip_tracer_series_read(RDyHipOperator op, int32_t first, int32_t count, double *times, double *values, void *stream) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  const TracerOutput &t = op->tracer_out;
  if (first < 0 || count < 0 || (int64_t)first + count > (int64_t)t.times.size())
    return fail(RDYHIP_ERR_USER, "tracer series: records [%d, %d + %d) are not in the log (%d records)", first, first, count, (int)t.times.size());
  const size_t row = (size_t)t.entries * (size_t)tout_width(op);
  if (count > 0 && (!times || (row > 0 && !values))) return fail(RDYHIP_ERR_USER, "null times / values");
  if (count == 0) return 0;
  std::copy(t.times.begin() + first, t.times.begin() + first + count, times);
  if (row > 0)
    HIP_TRY(hipMemcpyAsync(values, t.d_log.p + (size_t)first * row, sizeof(double) * (size_t)count * row, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

extern "C" int rdyhip_tracer_series_clear(RDyHipOperator op) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  op->tracer_out.times.clear();
  return 0;
}
