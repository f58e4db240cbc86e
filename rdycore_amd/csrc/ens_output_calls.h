// Output of the ensemble state behind the C ABI (rdyhip_ens_state_*, rdyhip_ens_error_sums*, rdyhip_ens_output_mean_*,
// rdyhip_ens_series_*, rdyhip_ens_stats; kernels: ens_output_kernels.h): the read-out, error sums, output means and observation
// series of readout_calls.h, output_calls.h and series_calls.h for all B members in one launch each, over the same helpers
// (output_shared.h), and the statistics over the members.  Included by rdyhip_api.hip only, after ensemble_calls.h (ensemble_check,
// ensemble_check_member) and readout_calls.h (READ_COMPS, one_component).
#pragma once
namespace {

// null operator, ensemble not enabled, then the mask: 1..7
int eout_check_comps(RDyHipOperator op, int32_t comps) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (comps < 1 || comps > READ_COMPS) return fail(RDYHIP_ERR_USER, "component mask 0x%x is not in 1..7 (RDYHIP_COMPONENT_*)", (unsigned)comps);
  return 0;
}
// ... the member, then exactly one component
int eout_check_member_comp(RDyHipOperator op, int32_t member, int32_t comp) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  if (!one_component(comp)) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comp);
  return 0;
}

dim3 eout_grid(RDyHipOperator op, int64_t n) { return dim3((unsigned)((n + ENS_OUT_BLOCK - 1) / ENS_OUT_BLOCK), (unsigned)op->ensemble.members); }

int launch_ens_planes(RDyHipOperator op, int32_t comps, const double *u, double *planes, hipStream_t st) {
  hipLaunchKernelGGL(ens_planes_kernel, eout_grid(op, op->n_owned), dim3(ENS_OUT_BLOCK), 0, st, op->n_owned, owned_to_local(op), (int)comps, popcount(comps),
                     3 * (int64_t)op->n_cells, (const uint64_t *)u, (uint64_t *)planes);
  HIP_TRY(hipGetLastError());
  return 0;
}

// null operator, ensemble not enabled, unknown bits, not exactly one variable: the argument errors the five mean calls share
int eout_means_check(RDyHipOperator op, int32_t vars, bool single) {
  int rc = ensemble_check(op);
  return rc ? rc : means_check_vars(vars, single);
}

int eout_series_check(RDyHipOperator op) {
  int rc = ensemble_check(op);
  return rc ? rc : series_check_enabled(op->ens_out.series, ENS_WORDS);
}

}  // namespace

extern "C" int rdyhip_ens_state_planes(RDyHipOperator op, int32_t comps, const double *u_local, double *d_planes, void *stream) {
  int rc = eout_check_comps(op, comps);
  if (rc) return rc;
  if (op->n_owned == 0) return 0;
  if (!u_local || !d_planes) return fail(RDYHIP_ERR_USER, "null u_local / d_planes");
  return launch_ens_planes(op, comps, u_local, d_planes, (hipStream_t)stream);
}

extern "C" int rdyhip_ens_state_read_begin(RDyHipOperator op, int32_t comps, const double *u_local, void *stream) {
  int rc = eout_check_comps(op, comps);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  return read_begin(op, op->ens_out.planes, comps, (size_t)op->ensemble.members * (size_t)popcount(comps) * (size_t)op->n_owned, u_local, st,
                    [&](double *planes) { return launch_ens_planes(op, comps, u_local, planes, st); });
}

extern "C" int rdyhip_ens_state_read_ready(RDyHipOperator op, int32_t *ready) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!ready) return fail(RDYHIP_ERR_USER, "null argument");
  return read_ready(op, op->ens_out.planes, ENS_WORDS, ready);
}

extern "C" int rdyhip_ens_state_read_wait(RDyHipOperator op) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  return read_wait(op, op->ens_out.planes, ENS_WORDS);
}

extern "C" int rdyhip_ens_state_read_get(RDyHipOperator op, int32_t member, int32_t comp, int32_t size, double *values) {
  int rc = eout_check_member_comp(op, member, comp);
  if (rc) return rc;
  return read_get(op, op->ens_out.planes, ENS_WORDS, member, comp, size, values);
}

extern "C" int rdyhip_ens_state_read_ptr(RDyHipOperator op, int32_t member, int32_t comp, const double **pinned_values) {
  int rc = eout_check_member_comp(op, member, comp);
  if (rc) return rc;
  if (!pinned_values) return fail(RDYHIP_ERR_USER, "null argument");
  return read_landed_plane(op, op->ens_out.planes, ENS_WORDS, member, comp, pinned_values);
}

extern "C" int rdyhip_ens_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int   B  = op->ensemble.members;
  // every member's workgroup records, then the B results: [B][err_wg + 1][10] as records of B x 10
  return sums_begin(op, op->ens_out.sums, (size_t)B * ERR_VALUES, u_local, st, [&](int wg, double *records, double *results) {
    hipLaunchKernelGGL(ens_error_partial_kernel, dim3(wg, B), dim3(ERR_BLOCK), 0, st, op->n_owned, owned_to_local(op), 3 * (int64_t)op->n_cells, u_local,
                       d_exact, (const double *)op->readout.d_area.p, records);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ens_error_finalize_kernel, dim3(B), dim3(ERR_BLOCK), 0, st, wg, (const double *)records, results);
    HIP_TRY(hipGetLastError());
    return 0;
  });
}

extern "C" int rdyhip_ens_error_sums_get(RDyHipOperator op, RDyHipErrorSums *out) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!out) return fail(RDYHIP_ERR_USER, "null argument");
  rc = sums_wait(op, op->ens_out.sums, ENS_WORDS);
  if (rc) return rc;
  static_assert(sizeof(RDyHipErrorSums) == sizeof(double) * ERR_VALUES, "RDyHipErrorSums is the ten doubles of a record");
  const size_t B = (size_t)op->ensemble.members;
  if (op->n_owned == 0) {
    memset(out, 0, sizeof(*out) * B);
  } else {
    memcpy(out, op->ens_out.sums.h_sums, sizeof(*out) * B);
  }
  return 0;
}

extern "C" int rdyhip_ens_output_mean_enable(RDyHipOperator op, int32_t vars) {
  int rc = eout_means_check(op, vars, false);
  if (rc) return rc;
  const size_t B = (size_t)op->ensemble.members;
  return means_enable(op->ens_out.means, vars, B * 3 * (size_t)op->n_owned, B);
}

extern "C" int rdyhip_ens_output_mean_accumulate(RDyHipOperator op, int32_t vars, const double *dts, const double *u_solution, const double *u_primitive,
                                                 void *stream) {
  int rc = eout_means_check(op, vars, false);
  if (!rc) rc = means_check_enabled(op->ens_out.means, ENS_WORDS, vars);
  if (rc) return rc;
  if (!dts) return fail(RDYHIP_ERR_USER, "null dts");
  const bool sol = vars & RDYHIP_OUTPUT_SOLUTION, prim = vars & RDYHIP_OUTPUT_PRIMITIVE_VARIABLES, src = vars & RDYHIP_OUTPUT_SOURCES;
  if (sol && op->n_owned > 0 && !u_solution) return fail(RDYHIP_ERR_USER, "null u_solution (needed with RDYHIP_OUTPUT_SOLUTION)");
  if (prim && op->n_owned > 0 && !u_primitive) return fail(RDYHIP_ERR_USER, "null u_primitive (needed with RDYHIP_OUTPUT_PRIMITIVE_VARIABLES)");
  OutputMeans &t = op->ens_out.means;
  const int    B = op->ensemble.members;
  if (op->n_owned > 0 && vars) {
    EnsPerMember d{};
    for (int m = 0; m < B; ++m) d.v[m] = dts[m];
    // the sources: the members' own [B][owned][3] array, read at this place in the stream
    const double *us = sol ? u_solution : nullptr, *up = prim ? u_primitive : nullptr, *ext = src ? op->ensemble.extsrc.p : nullptr;
    double       *acc_s = sol ? t.acc[0].p : nullptr, *acc_p = prim ? t.acc[1].p : nullptr, *acc_x = src ? t.acc[2].p : nullptr;
    const double  tiny_h = op->config.tiny_h, ha2 = op->config.h_anuga_regular * op->config.h_anuga_regular;
    hipLaunchKernelGGL(ens_output_accumulate_kernel, eout_grid(op, op->n_owned), dim3(ENS_OUT_BLOCK), 0, (hipStream_t)stream, op->n_owned, owned_to_local(op), d,
                       3 * (int64_t)op->n_cells, us, acc_s, up, tiny_h, ha2, acc_p, ext, acc_x);
    HIP_TRY(hipGetLastError());
  }
  for (int i = 0; i < 3; ++i)
    if (vars >> i & 1)
      for (int m = 0; m < B; ++m) t.time[i][(size_t)m] += dts[m];   // AccumulateOutputVar: accumulated_time += dt, per member
  return 0;
}

extern "C" int rdyhip_ens_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean, double *accumulated_times, void *stream) {
  int rc = eout_means_check(op, var, true);
  if (!rc) rc = means_check_enabled(op->ens_out.means, ENS_WORDS, var);
  if (rc) return rc;
  const int          i = output_index(var), B = op->ensemble.members;
  const OutputMeans &t = op->ens_out.means;
  if (op->n_owned > 0 && !d_mean) return fail(RDYHIP_ERR_USER, "null d_mean");
  // ComputeMean's PetscCheck (src/xdmf_output.c:213), for every member before anything is launched or written
  for (int m = 0; m < B; ++m)
    if (!(t.time[i][(size_t)m] > 0.0))
      return fail(RDYHIP_ERR_USER, "ensemble output variable 0x%x: member %d has no accumulated time", (unsigned)var, m);
  EnsPerMember s{};
  for (int m = 0; m < B; ++m) {
    if (accumulated_times) accumulated_times[m] = t.time[i][(size_t)m];
    s.v[m] = 1.0 / t.time[i][(size_t)m];
  }
  const int64_t n = 3 * (int64_t)op->n_owned;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ens_output_mean_kernel, eout_grid(op, n), dim3(ENS_OUT_BLOCK), 0, (hipStream_t)stream, n, s, (const double *)t.acc[i].p, d_mean);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int rdyhip_ens_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream) {
  int rc = eout_means_check(op, vars, false);
  if (!rc) rc = means_check_enabled(op->ens_out.means, ENS_WORDS, vars);
  if (rc) return rc;
  return means_reset(op, op->ens_out.means, vars, (hipStream_t)stream);
}

extern "C" int rdyhip_ens_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_times) {
  int rc = eout_means_check(op, var, true);
  if (rc) return rc;
  if (!accumulated_times) return fail(RDYHIP_ERR_USER, "null accumulated_times");
  return means_time(op->ens_out.means, ENS_WORDS, var, accumulated_times);
}

extern "C" int rdyhip_ens_series_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids, int32_t capacity) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  std::vector<int32_t> local;
  rc = series_sites(op, op->ens_out.series, ENS_WORDS, num_sites, owned_cell_ids, capacity, local);
  if (rc) return rc;
  const size_t B = (size_t)op->ensemble.members;
  SeriesLog    s;
  rc = s.d_sites.upload(local);
  if (!rc) rc = series_alloc_log(&s, num_sites, capacity, B * 3, B);
  if (!rc) op->ens_out.series = std::move(s);
  return rc;
}

extern "C" int rdyhip_ens_series_record(RDyHipOperator op, const double *times, const double *u_local, void *stream) {
  int rc = eout_series_check(op);
  if (rc) return rc;
  SeriesLog &t = op->ens_out.series;
  if (!times) return fail(RDYHIP_ERR_USER, "null times");
  if (t.entries > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  rc = series_check_room(t, ENS_WORDS);
  if (rc) return rc;
  const int B = op->ensemble.members;
  if (t.entries > 0) {
    hipLaunchKernelGGL(ens_series_observe_kernel, eout_grid(op, t.entries), dim3(ENS_OUT_BLOCK), 0, (hipStream_t)stream, t.entries, B,
                       (const int32_t *)t.d_sites.p, 3 * (int64_t)op->n_cells, u_local, (int64_t)t.records, t.d_log.p);
    HIP_TRY(hipGetLastError());
  }
  t.times.insert(t.times.end(), times, times + B);
  ++t.records;
  return 0;
}

extern "C" int rdyhip_ens_series_info(RDyHipOperator op, int32_t *entries, int32_t *count, int32_t *capacity) {
  int rc = eout_series_check(op);
  if (rc) return rc;
  series_info(op->ens_out.series, entries, count, capacity);
  return 0;
}

extern "C" int rdyhip_ens_series_read(RDyHipOperator op, int32_t first, int32_t count, double *times, double *values, void *stream) {
  int rc = eout_series_check(op);
  if (rc) return rc;
  const SeriesLog &t = op->ens_out.series;
  const size_t     B = (size_t)op->ensemble.members;
  return series_read(t, "ensemble series", B * (size_t)t.entries * 3, B, first, count, times, values, (hipStream_t)stream);
}

extern "C" int rdyhip_ens_series_clear(RDyHipOperator op) {
  int rc = eout_series_check(op);
  if (rc) return rc;
  series_clear(op->ens_out.series);
  return 0;
}

extern "C" int rdyhip_ens_stats(RDyHipOperator op, int32_t comps, const double *u_local, double *d_stats, void *stream) {
  int rc = eout_check_comps(op, comps);
  if (rc) return rc;
  if (op->n_owned == 0) return 0;
  if (!u_local || !d_stats) return fail(RDYHIP_ERR_USER, "null u_local / d_stats");
  const int B = op->ensemble.members;
  hipLaunchKernelGGL(ens_stats_kernel, dim3((unsigned)((op->n_owned + ENS_OUT_BLOCK - 1) / ENS_OUT_BLOCK)), dim3(ENS_OUT_BLOCK), 0, (hipStream_t)stream,
                     op->n_owned, owned_to_local(op), (int)comps, B, 1.0 / (double)B, 3 * (int64_t)op->n_cells, u_local, d_stats);
  HIP_TRY(hipGetLastError());
  return 0;
}
