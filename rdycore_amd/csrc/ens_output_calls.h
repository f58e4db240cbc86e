// Output of the ensemble state behind the C ABI (rdyhip_ens_state_*, rdyhip_ens_error_sums*, rdyhip_ens_output_mean_*,
// rdyhip_ens_series_*, rdyhip_ens_stats; kernels: ens_output_kernels.h): the read-out, error sums, output means and observation
// series of readout_calls.h, output_calls.h and series_calls.h for all B members in one launch each, and the statistics over the
// members.  Included by rdyhip_api.hip only, after ensemble_calls.h (ensemble_check, ensemble_check_member) and those three
// (READ_COMPS, popcount3, one_component, sums_reserve, OUT_VARS, output_index).
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

const int32_t *eout_o2l(RDyHipOperator op) { return op->prefix ? (const int32_t *)nullptr : op->d_o2l.p; }
dim3 eout_grid(RDyHipOperator op, int64_t n) { return dim3((unsigned)((n + ENS_OUT_BLOCK - 1) / ENS_OUT_BLOCK), (unsigned)op->ensemble.members); }

int launch_ens_planes(RDyHipOperator op, int32_t comps, const double *u, double *planes, hipStream_t st) {
  hipLaunchKernelGGL(ens_planes_kernel, eout_grid(op, op->n_owned), dim3(ENS_OUT_BLOCK), 0, st, op->n_owned, eout_o2l(op), (int)comps, popcount3(comps),
                     3 * (int64_t)op->n_cells, (const uint64_t *)u, (uint64_t *)planes);
  HIP_TRY(hipGetLastError());
  return 0;
}

// read_reserve (readout_calls.h) for the ensemble read-out's own buffers and events: B x k planes; the copy stream is the operator's
int eout_read_reserve(RDyHipOperator op, int k) {
  EnsembleOutput &r = op->ens_out;
  if (!op->stage.copy) HIP_TRY(hipStreamCreateWithFlags(&op->stage.copy, hipStreamNonBlocking));
  if (!r.launched) HIP_TRY(hipEventCreateWithFlags(&r.launched, hipEventDisableTiming));
  if (!r.done) HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  const size_t need = (size_t)op->ensemble.members * (size_t)k * (size_t)op->n_owned;
  if (r.d_planes.p && r.d_planes.n >= need && r.h_cap >= need) return 0;
  if (r.state == EnsembleOutput::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.done));
  r.state = EnsembleOutput::NONE;   // whatever had been read lived in the old buffers
  int rc = r.d_planes.alloc(need);
  if (rc) return rc;
  if (r.h_planes) HIP_TRY(hipHostFree(r.h_planes));
  r.h_planes = nullptr;
  r.h_cap    = 0;
  HIP_TRY(hipHostMalloc((void **)&r.h_planes, sizeof(double) * need, hipHostMallocDefault));
  r.h_cap = need;
  return 0;
}

// the state checks of _get and _ptr; *plane = the index of (member, comp) among the planes of the last begin
int eout_check_landed(RDyHipOperator op, int32_t member, int32_t comp, size_t *plane) {
  const EnsembleOutput &r = op->ens_out;
  if (r.state != EnsembleOutput::LANDED)
    return fail(RDYHIP_ERR_USER, r.state == EnsembleOutput::NONE ? "no ensemble state read has been begun (rdyhip_ens_state_read_begin)"
                                                                 : "the ensemble state read has not been waited for (rdyhip_ens_state_read_wait)");
  if (!(r.comps & comp))
    return fail(RDYHIP_ERR_USER, "component 0x%x was not asked for by the last rdyhip_ens_state_read_begin (0x%x)", (unsigned)comp, (unsigned)r.comps);
  *plane = (size_t)member * (size_t)popcount3(r.comps) + (size_t)popcount3(r.comps & (comp - 1));
  return 0;
}

// the shared area table (and the workgroup count that goes with n_owned), this feature's records and pinned results
int eout_sums_reserve(RDyHipOperator op) {
  int rc = sums_reserve(op);
  if (rc) return rc;
  EnsembleOutput &r = op->ens_out;
  const size_t    B = (size_t)op->ensemble.members;
  if (!r.sums_done) HIP_TRY(hipEventCreateWithFlags(&r.sums_done, hipEventDisableTiming));
  if (!r.h_sums) HIP_TRY(hipHostMalloc((void **)&r.h_sums, sizeof(double) * B * ERR_VALUES, hipHostMallocDefault));
  if (!r.d_records.p) {
    DevBuf<double> records;
    rc = records.alloc(B * (size_t)(op->readout.err_wg + 1) * ERR_VALUES);
    if (rc) return rc;
    r.d_records = std::move(records);
  }
  return 0;
}

// null operator, ensemble not enabled, unknown bits, not exactly one variable: the argument errors the five mean calls share
int eout_means_check(RDyHipOperator op, int32_t vars, bool single) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (vars & ~OUT_VARS) return fail(RDYHIP_ERR_USER, "unknown output variable bits 0x%x", (unsigned)(vars & ~OUT_VARS));
  if (single && vars != RDYHIP_OUTPUT_SOLUTION && vars != RDYHIP_OUTPUT_PRIMITIVE_VARIABLES && vars != RDYHIP_OUTPUT_SOURCES)
    return fail(RDYHIP_ERR_USER, "exactly one output variable is needed (got 0x%x)", (unsigned)vars);
  return 0;
}
int eout_means_check_enabled(RDyHipOperator op, int32_t vars) {
  for (int i = 0; i < 3; ++i)
    if ((vars >> i & 1) && !op->ens_out.acc[i].p)
      return fail(RDYHIP_ERR_USER, "ensemble output variable 0x%x is not enabled (rdyhip_ens_output_mean_enable)", 1u << i);
  return 0;
}

int eout_series_check(RDyHipOperator op) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!op->ens_out.series_enabled) return fail(RDYHIP_ERR_USER, "the ensemble observation series is not enabled (rdyhip_ens_series_enable)");
  return 0;
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
  EnsembleOutput &r = op->ens_out;
  if (op->n_owned == 0) {   // nothing is launched or copied: the read has landed as soon as it is waited for
    r.comps = comps;
    r.state = EnsembleOutput::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  hipStream_t st = (hipStream_t)stream;
  const int   k  = popcount3(comps);
  rc = eout_read_reserve(op, k);
  if (rc) return rc;
  // an earlier read that has not landed is given up; its copy may still be reading the device planes, so this launch waits for it
  if (r.state == EnsembleOutput::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.done, 0));
  r.state = EnsembleOutput::NONE;
  rc = launch_ens_planes(op, comps, u_local, r.d_planes.p, st);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(r.launched, st));
  HIP_TRY(hipStreamWaitEvent(op->stage.copy, r.launched, 0));
  HIP_TRY(hipMemcpyAsync(r.h_planes, r.d_planes.p, sizeof(double) * (size_t)op->ensemble.members * (size_t)k * (size_t)op->n_owned, hipMemcpyDeviceToHost,
                         op->stage.copy));
  HIP_TRY(hipEventRecord(r.done, op->stage.copy));
  r.comps = comps;
  r.state = EnsembleOutput::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_ens_state_read_ready(RDyHipOperator op, int32_t *ready) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!ready) return fail(RDYHIP_ERR_USER, "null argument");
  const EnsembleOutput &r = op->ens_out;
  if (r.state == EnsembleOutput::NONE) return fail(RDYHIP_ERR_USER, "no ensemble state read has been begun (rdyhip_ens_state_read_begin)");
  *ready = 1;
  if (r.state == EnsembleOutput::IN_FLIGHT && op->n_owned > 0) {
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

extern "C" int rdyhip_ens_state_read_wait(RDyHipOperator op) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  EnsembleOutput &r = op->ens_out;
  if (r.state == EnsembleOutput::NONE) return fail(RDYHIP_ERR_USER, "no ensemble state read has been begun (rdyhip_ens_state_read_begin)");
  if (r.state == EnsembleOutput::IN_FLIGHT && op->n_owned > 0) HIP_TRY(hipEventSynchronize(r.done));
  r.state = EnsembleOutput::LANDED;
  return 0;
}

extern "C" int rdyhip_ens_state_read_get(RDyHipOperator op, int32_t member, int32_t comp, int32_t size, double *values) {
  int rc = eout_check_member_comp(op, member, comp);
  if (rc) return rc;
  // CheckNumOwnedCells (src/rdydata.c:54-58)
  if (size != op->n_owned) return fail(RDYHIP_ERR_ARG_SIZ, "The size of array (%d) is not equal to the number of owned cells (%d)", size, op->n_owned);
  if (size > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  size_t plane = 0;
  rc = eout_check_landed(op, member, comp, &plane);
  if (rc) return rc;
  if (size > 0) memcpy(values, op->ens_out.h_planes + plane * (size_t)op->n_owned, sizeof(double) * (size_t)size);
  return 0;
}

extern "C" int rdyhip_ens_state_read_ptr(RDyHipOperator op, int32_t member, int32_t comp, const double **pinned_values) {
  int rc = eout_check_member_comp(op, member, comp);
  if (rc) return rc;
  if (!pinned_values) return fail(RDYHIP_ERR_USER, "null argument");
  size_t plane = 0;
  rc = eout_check_landed(op, member, comp, &plane);
  if (rc) return rc;
  *pinned_values = op->n_owned > 0 ? op->ens_out.h_planes + plane * (size_t)op->n_owned : nullptr;
  return 0;
}

extern "C" int rdyhip_ens_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  EnsembleOutput &r = op->ens_out;
  if (op->n_owned == 0) {   // all zeros, nothing launched
    r.sums_state = EnsembleOutput::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  rc = eout_sums_reserve(op);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the records and the pinned results are shared by all calls: this one is ordered behind an earlier one that is still running
  if (r.sums_state == EnsembleOutput::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.sums_done, 0));
  const int    wg = op->readout.err_wg, B = op->ensemble.members;
  double      *results = r.d_records.p + (size_t)B * (size_t)wg * ERR_VALUES;
  hipLaunchKernelGGL(ens_error_partial_kernel, dim3(wg, B), dim3(ERR_BLOCK), 0, st, op->n_owned, eout_o2l(op), 3 * (int64_t)op->n_cells, u_local, d_exact,
                     (const double *)op->readout.d_area.p, r.d_records.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ens_error_finalize_kernel, dim3(B), dim3(ERR_BLOCK), 0, st, wg, (const double *)r.d_records.p, results);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(r.h_sums, results, sizeof(double) * (size_t)B * ERR_VALUES, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(r.sums_done, st));
  r.sums_state = EnsembleOutput::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_ens_error_sums_get(RDyHipOperator op, RDyHipErrorSums *out) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!out) return fail(RDYHIP_ERR_USER, "null argument");
  EnsembleOutput &r = op->ens_out;
  if (r.sums_state == EnsembleOutput::NONE) return fail(RDYHIP_ERR_USER, "no ensemble error sums have been asked for (rdyhip_ens_error_sums)");
  static_assert(sizeof(RDyHipErrorSums) == sizeof(double) * ERR_VALUES, "RDyHipErrorSums is the ten doubles of a record");
  const size_t B = (size_t)op->ensemble.members;
  if (op->n_owned == 0) {
    memset(out, 0, sizeof(*out) * B);
  } else {
    if (r.sums_state == EnsembleOutput::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.sums_done));
    memcpy(out, r.h_sums, sizeof(*out) * B);
  }
  r.sums_state = EnsembleOutput::LANDED;
  return 0;
}

extern "C" int rdyhip_ens_output_mean_enable(RDyHipOperator op, int32_t vars) {
  int rc = eout_means_check(op, vars, false);
  if (rc) return rc;
  const size_t B = (size_t)op->ensemble.members;
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1) || op->ens_out.acc[i].p) continue;   // an existing accumulator keeps its content
    DevBuf<double> a;
    rc = a.zeros(B * 3 * (size_t)op->n_owned);
    if (rc) return rc;
    op->ens_out.acc[i] = std::move(a);
    op->ens_out.time[i].assign(B, 0.0);
  }
  return 0;
}

extern "C" int rdyhip_ens_output_mean_accumulate(RDyHipOperator op, int32_t vars, const double *dts, const double *u_solution, const double *u_primitive,
                                                 void *stream) {
  int rc = eout_means_check(op, vars, false);
  if (!rc) rc = eout_means_check_enabled(op, vars);
  if (rc) return rc;
  if (!dts) return fail(RDYHIP_ERR_USER, "null dts");
  const bool sol = vars & RDYHIP_OUTPUT_SOLUTION, prim = vars & RDYHIP_OUTPUT_PRIMITIVE_VARIABLES, src = vars & RDYHIP_OUTPUT_SOURCES;
  if (sol && op->n_owned > 0 && !u_solution) return fail(RDYHIP_ERR_USER, "null u_solution (needed with RDYHIP_OUTPUT_SOLUTION)");
  if (prim && op->n_owned > 0 && !u_primitive) return fail(RDYHIP_ERR_USER, "null u_primitive (needed with RDYHIP_OUTPUT_PRIMITIVE_VARIABLES)");
  EnsembleOutput &t = op->ens_out;
  const int       B = op->ensemble.members;
  if (op->n_owned > 0 && vars) {
    EnsPerMember d{};
    for (int m = 0; m < B; ++m) d.v[m] = dts[m];
    // the sources: the members' own [B][owned][3] array, read at this place in the stream
    const double *us = sol ? u_solution : nullptr, *up = prim ? u_primitive : nullptr, *ext = src ? op->ensemble.extsrc.p : nullptr;
    double       *acc_s = sol ? t.acc[0].p : nullptr, *acc_p = prim ? t.acc[1].p : nullptr, *acc_x = src ? t.acc[2].p : nullptr;
    const double  tiny_h = op->config.tiny_h, ha2 = op->config.h_anuga_regular * op->config.h_anuga_regular;
    hipLaunchKernelGGL(ens_output_accumulate_kernel, eout_grid(op, op->n_owned), dim3(ENS_OUT_BLOCK), 0, (hipStream_t)stream, op->n_owned, eout_o2l(op), d,
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
  if (!rc) rc = eout_means_check_enabled(op, var);
  if (rc) return rc;
  const int       i = output_index(var), B = op->ensemble.members;
  EnsembleOutput &t = op->ens_out;
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
  if (!rc) rc = eout_means_check_enabled(op, vars);
  if (rc) return rc;
  EnsembleOutput &t = op->ens_out;
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1)) continue;
    if (op->n_owned > 0) HIP_TRY(hipMemsetAsync(t.acc[i].p, 0, t.acc[i].bytes(), (hipStream_t)stream));
    std::fill(t.time[i].begin(), t.time[i].end(), 0.0);
  }
  return 0;
}

extern "C" int rdyhip_ens_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_times) {
  int rc = eout_means_check(op, var, true);
  if (rc) return rc;
  if (!accumulated_times) return fail(RDYHIP_ERR_USER, "null accumulated_times");
  rc = eout_means_check_enabled(op, var);
  if (rc) return rc;
  const std::vector<double> &t = op->ens_out.time[output_index(var)];
  std::copy(t.begin(), t.end(), accumulated_times);
  return 0;
}

extern "C" int rdyhip_ens_series_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids, int32_t capacity) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (num_sites < 0 || capacity < 0) return fail(RDYHIP_ERR_USER, "negative number of sites (%d) or capacity (%d)", num_sites, capacity);
  if (num_sites > 0 && !owned_cell_ids) return fail(RDYHIP_ERR_USER, "null owned_cell_ids");
  EnsembleOutput &t = op->ens_out;
  if (t.series_enabled) return fail(RDYHIP_ERR_USER, "the ensemble observation series is enabled already");
  for (int32_t i = 0; i < num_sites; ++i)
    if (owned_cell_ids[i] < 0 || owned_cell_ids[i] >= op->n_owned)
      return fail(RDYHIP_ERR_USER, "observation site %d: owned cell %d out of range [0, %d)", i, owned_cell_ids[i], op->n_owned);
  std::vector<int32_t> local(owned_cell_ids, owned_cell_ids + num_sites);
  if (!op->prefix && num_sites > 0) {   // owned -> local through the operator's own table
    std::vector<int32_t> o2l((size_t)op->n_owned);
    HIP_TRY(hipMemcpy(o2l.data(), op->d_o2l.p, sizeof(int32_t) * (size_t)op->n_owned, hipMemcpyDeviceToHost));
    for (auto &c : local) c = o2l[(size_t)c];
  }
  const size_t    B = (size_t)op->ensemble.members;
  DevBuf<int32_t> sites;
  DevBuf<double>  log;
  rc = sites.upload(local);
  if (!rc) rc = log.zeros((size_t)capacity * B * (size_t)num_sites * 3);
  if (rc) return rc;
  t.d_sites  = std::move(sites);
  t.d_log    = std::move(log);
  t.entries  = num_sites;
  t.capacity = capacity;
  t.records  = 0;
  t.times.clear();
  t.times.reserve((size_t)capacity * B);
  t.series_enabled = true;
  return 0;
}

extern "C" int rdyhip_ens_series_record(RDyHipOperator op, const double *times, const double *u_local, void *stream) {
  int rc = eout_series_check(op);
  if (rc) return rc;
  EnsembleOutput &t = op->ens_out;
  if (!times) return fail(RDYHIP_ERR_USER, "null times");
  if (t.entries > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  if (t.records >= t.capacity)
    return fail(RDYHIP_ERR_USER, "ensemble series: the log is full (%d records); read it and call rdyhip_ens_series_clear", t.capacity);
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
  const EnsembleOutput &t = op->ens_out;
  if (entries) *entries = t.entries;
  if (count) *count = t.records;
  if (capacity) *capacity = t.capacity;
  return 0;
}

extern "C" int rdyhip_ens_series_read(RDyHipOperator op, int32_t first, int32_t count, double *times, double *values, void *stream) {
  int rc = eout_series_check(op);
  if (rc) return rc;
  const EnsembleOutput &t = op->ens_out;
  if (first < 0 || count < 0 || (int64_t)first + count > (int64_t)t.records)
    return fail(RDYHIP_ERR_USER, "ensemble series: records [%d, %d + %d) are not in the log (%d records)", first, first, count, t.records);
  const size_t B = (size_t)op->ensemble.members, row = B * (size_t)t.entries * 3;
  if (count > 0 && (!times || (row > 0 && !values))) return fail(RDYHIP_ERR_USER, "null times / values");
  if (count == 0) return 0;
  std::copy(t.times.begin() + (size_t)first * B, t.times.begin() + ((size_t)first + (size_t)count) * B, times);
  if (row > 0)
    HIP_TRY(hipMemcpyAsync(values, t.d_log.p + (size_t)first * row, sizeof(double) * (size_t)count * row, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

extern "C" int rdyhip_ens_series_clear(RDyHipOperator op) {
  int rc = eout_series_check(op);
  if (rc) return rc;
  op->ens_out.times.clear();
  op->ens_out.records = 0;
  return 0;
}

extern "C" int rdyhip_ens_stats(RDyHipOperator op, int32_t comps, const double *u_local, double *d_stats, void *stream) {
  int rc = eout_check_comps(op, comps);
  if (rc) return rc;
  if (op->n_owned == 0) return 0;
  if (!u_local || !d_stats) return fail(RDYHIP_ERR_USER, "null u_local / d_stats");
  const int B = op->ensemble.members;
  hipLaunchKernelGGL(ens_stats_kernel, dim3((unsigned)((op->n_owned + ENS_OUT_BLOCK - 1) / ENS_OUT_BLOCK)), dim3(ENS_OUT_BLOCK), 0, (hipStream_t)stream,
                     op->n_owned, eout_o2l(op), (int)comps, B, 1.0 / (double)B, 3 * (int64_t)op->n_cells, u_local, d_stats);
  HIP_TRY(hipGetLastError());
  return 0;
}
