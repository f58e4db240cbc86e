// Output of the tracer state behind the C ABI (rdyhip_tracer_state_*, rdyhip_tracer_error_sums*, rdyhip_tracer_output_mean_*,
// rdyhip_tracer_series_*; kernels: tracer_output_kernels.h): the read-out, error sums, output means and observation series of
// readout_calls.h, output_calls.h and series_calls.h for rows of N = 3 + NT, over the same helpers (output_shared.h).  Included by
// rdyhip_api.hip only, after tracer_calls.h (tracers_check).
#pragma once
namespace {

int tout_width(RDyHipOperator op) { return 3 + op->tracers.n; }

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
  const int32_t *o2l = owned_to_local(op);
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

// null operator, tracers not enabled, unknown bits, not exactly one variable: the argument errors the five mean calls share
int tout_means_check(RDyHipOperator op, int32_t vars, bool single) {
  int rc = tracers_check(op);
  return rc ? rc : means_check_vars(vars, single);
}

int tout_series_check(RDyHipOperator op) {
  int rc = tracers_check(op);
  return rc ? rc : series_check_enabled(op->tracer_out.series, TRACER_WORDS);
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
  hipStream_t st = (hipStream_t)stream;
  return read_begin(op, op->tracer_out.planes, comps, (size_t)popcount(comps) * (size_t)op->n_owned, u_local, st,
                    [&](double *planes) { return launch_tracer_planes(op, comps, form, u_local, planes, st); });
}

extern "C" int rdyhip_tracer_state_read_ready(RDyHipOperator op, int32_t *ready) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!ready) return fail(RDYHIP_ERR_USER, "null argument");
  return read_ready(op, op->tracer_out.planes, TRACER_WORDS, ready);
}

extern "C" int rdyhip_tracer_state_read_wait(RDyHipOperator op) {
  int rc = tracers_check(op);
  if (rc) return rc;
  return read_wait(op, op->tracer_out.planes, TRACER_WORDS);
}

extern "C" int rdyhip_tracer_state_read_get(RDyHipOperator op, int32_t comp, int32_t size, double *values) {
  int rc = tout_check_comps(op, comp, true);
  if (rc) return rc;
  return read_get(op, op->tracer_out.planes, TRACER_WORDS, 0, comp, size, values);
}

extern "C" int rdyhip_tracer_state_read_ptr(RDyHipOperator op, int32_t comp, const double **pinned_values) {
  int rc = tout_check_comps(op, comp, true);
  if (rc) return rc;
  if (!pinned_values) return fail(RDYHIP_ERR_USER, "null argument");
  return read_landed_plane(op, op->tracer_out.planes, TRACER_WORDS, 0, comp, pinned_values);
}

extern "C" int rdyhip_tracer_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream) {
  int rc = tracers_check(op);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  return sums_begin(op, op->tracer_out.sums, 3 * (size_t)tout_width(op) + 1, u_local, st, [&](int wg, double *records, double *result) {
    return with_tracer_count(op->tracers.n, [&](auto nt) {
      constexpr int NT = decltype(nt)::value;
      hipLaunchKernelGGL((tracer_error_partial_kernel<NT>), dim3(wg), dim3(ERR_BLOCK), 0, st, op->n_owned, owned_to_local(op), u_local, d_exact,
                         op->readout.d_area.p, records);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL((tracer_error_finalize_kernel<NT>), dim3(1), dim3(ERR_BLOCK), 0, st, wg, records, result);
      HIP_TRY(hipGetLastError());
      return 0;
    });
  });
}

extern "C" int rdyhip_tracer_error_sums_get(RDyHipOperator op, RDyHipTracerErrorSums *out) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!out) return fail(RDYHIP_ERR_USER, "null argument");
  rc = sums_wait(op, op->tracer_out.sums, TRACER_WORDS);
  if (rc) return rc;
  static_assert(sizeof(RDyHipTracerErrorSums) == sizeof(double) * (3 * (3 + RDYHIP_MAX_TRACERS) + 1), "three arrays of the widest row and the area");
  memset(out, 0, sizeof(*out));   // entries >= N stay 0
  if (op->n_owned > 0) {
    const double *h = op->tracer_out.sums.h_sums;
    const int     N = tout_width(op);
    for (int c = 0; c < N; ++c) {
      out->l1[c]         = h[c];
      out->l2_squared[c] = h[N + c];
      out->linf[c]       = h[2 * N + c];
    }
    out->area = h[3 * N];
  }
  return 0;
}

extern "C" int rdyhip_tracer_output_mean_enable(RDyHipOperator op, int32_t vars) {
  int rc = tout_means_check(op, vars, false);
  if (rc) return rc;
  return means_enable(op->tracer_out.means, vars, (size_t)tout_width(op) * op->n_owned, 1);
}

extern "C" int rdyhip_tracer_output_mean_accumulate(RDyHipOperator op, int32_t vars, double dt, const double *u_solution, const double *u_primitive,
                                                    void *stream) {
  int rc = tout_means_check(op, vars, false);
  if (!rc) rc = means_check_enabled(op->tracer_out.means, TRACER_WORDS, vars);
  if (rc) return rc;
  const bool sol = vars & RDYHIP_OUTPUT_SOLUTION, prim = vars & RDYHIP_OUTPUT_PRIMITIVE_VARIABLES, src = vars & RDYHIP_OUTPUT_SOURCES;
  if (sol && op->n_owned > 0 && !u_solution) return fail(RDYHIP_ERR_USER, "null u_solution (needed with RDYHIP_OUTPUT_SOLUTION)");
  if (prim && op->n_owned > 0 && !u_primitive) return fail(RDYHIP_ERR_USER, "null u_primitive (needed with RDYHIP_OUTPUT_PRIMITIVE_VARIABLES)");
  OutputMeans &t = op->tracer_out.means;
  if (op->n_owned > 0 && vars) {
    // the sources: the canonical [owned][3] array, which every writer keeps current whatever the water-only and uniform modes of
    // the SWE kernels are (operator_state.h), and the tracers' [owned][NT]; both read at this place in the stream
    const double *us = sol ? u_solution : nullptr, *up = prim ? u_primitive : nullptr;
    double       *acc_s = sol ? t.acc[0].p : nullptr, *acc_p = prim ? t.acc[1].p : nullptr, *acc_x = src ? t.acc[2].p : nullptr;
    const double  tiny_h = op->config.tiny_h, ha2 = op->config.h_anuga_regular * op->config.h_anuga_regular;
    const int32_t *o2l = owned_to_local(op);
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
    if (vars >> i & 1) t.time[i][0] += dt;   // AccumulateOutputVar: accumulated_time += dt
  return 0;
}

extern "C" int rdyhip_tracer_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean, double *accumulated_time, void *stream) {
  int rc = tout_means_check(op, var, true);
  if (!rc) rc = means_check_enabled(op->tracer_out.means, TRACER_WORDS, var);
  if (rc) return rc;
  return means_get(op, op->tracer_out.means, TRACER_WORDS, var, tout_width(op), d_mean, accumulated_time, (hipStream_t)stream);
}

extern "C" int rdyhip_tracer_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream) {
  int rc = tout_means_check(op, vars, false);
  if (!rc) rc = means_check_enabled(op->tracer_out.means, TRACER_WORDS, vars);
  if (rc) return rc;
  return means_reset(op, op->tracer_out.means, vars, (hipStream_t)stream);
}

extern "C" int rdyhip_tracer_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_time) {
  int rc = tout_means_check(op, var, true);
  if (rc) return rc;
  if (!accumulated_time) return fail(RDYHIP_ERR_USER, "null accumulated_time");
  return means_time(op->tracer_out.means, TRACER_WORDS, var, accumulated_time);
}

extern "C" int rdyhip_tracer_series_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids, int32_t capacity) {
  int rc = tracers_check(op);
  if (rc) return rc;
  std::vector<int32_t> local;
  rc = series_sites(op, op->tracer_out.series, TRACER_WORDS, num_sites, owned_cell_ids, capacity, local);
  if (rc) return rc;
  SeriesLog s;
  rc = s.d_sites.upload(local);
  if (!rc) rc = series_alloc_log(&s, num_sites, capacity, (size_t)tout_width(op));
  if (!rc) op->tracer_out.series = std::move(s);
  return rc;
}

extern "C" int rdyhip_tracer_series_record(RDyHipOperator op, double time, const double *u_local, void *stream) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  SeriesLog &t = op->tracer_out.series;
  if (t.entries > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  rc = series_check_room(t, TRACER_WORDS);
  if (rc) return rc;
  const int64_t r = t.records;
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
  ++t.records;
  return 0;
}

extern "C" int rdyhip_tracer_series_info(RDyHipOperator op, int32_t *entries, int32_t *count, int32_t *capacity) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  series_info(op->tracer_out.series, entries, count, capacity);
  return 0;
}

extern "C" int rdyhip_tracer_series_read(RDyHipOperator op, int32_t first, int32_t count, double *times, double *values, void *stream) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  const SeriesLog &t = op->tracer_out.series;
  return series_read(t, "tracer series", (size_t)t.entries * (size_t)tout_width(op), 1, first, count, times, values, (hipStream_t)stream);
}

extern "C" int rdyhip_tracer_series_clear(RDyHipOperator op) {
  int rc = tout_series_check(op);
  if (rc) return rc;
  series_clear(op->tracer_out.series);
  return 0;
}
