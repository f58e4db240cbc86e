// What the output calls of the three states share (readout_calls.h, output_calls.h, series_calls.h for the SWE state,
// tracer_output_calls.h, ens_output_calls.h): the host side of a plane read, of the error sums, of the output means and of an
// observation series, each written once over the pieces of operator_state.h.  What differs between the states goes in as a value
// (a width, a count of doubles, the words of a message) or as the callable that launches the state's kernel.  Included by
// rdyhip_api.hip only, after rk_calls.h (aligned16) and before the *_calls.h files above.
#pragma once
namespace {

// The words by which the messages of a state differ: its noun and the prefix of its entry points after "rdyhip_"
struct OutputWords {
  const char *noun, *fn;
};
constexpr OutputWords SWE_WORDS{"", ""}, TRACER_WORDS{"tracer ", "tracer_"}, ENS_WORDS{"ensemble ", "ens_"};

constexpr int32_t OUT_VARS = RDYHIP_OUTPUT_SOLUTION | RDYHIP_OUTPUT_PRIMITIVE_VARIABLES | RDYHIP_OUTPUT_SOURCES;

int popcount(int32_t comps) { return __builtin_popcount((unsigned)comps); }
int output_index(int32_t var) { return var == RDYHIP_OUTPUT_SOLUTION ? 0 : var == RDYHIP_OUTPUT_PRIMITIVE_VARIABLES ? 1 : 2; }

// ---- plane read ---------------------------------------------------------------------------------------------------------------

// the copy stream (shared with the setters' staging ring), the two events, and room for `need` doubles on the device and in pinned
// memory: grows only; a call that allocates may synchronise, and waits first for a copy that still reads the old buffers
int read_reserve(RDyHipOperator op, PlaneRead &r, size_t need) {
  if (!op->stage.copy) HIP_TRY(hipStreamCreateWithFlags(&op->stage.copy, hipStreamNonBlocking));
  if (!r.launched) HIP_TRY(hipEventCreateWithFlags(&r.launched, hipEventDisableTiming));
  if (!r.done) HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  if (r.d_planes.p && r.d_planes.n >= need && r.h_cap >= need) return 0;
  if (r.state == PlaneRead::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.done));
  r.state = PlaneRead::NONE;   // whatever had been read lived in the old buffers
  int rc = r.d_planes.alloc(need);
  if (rc) return rc;
  if (r.h_planes) HIP_TRY(hipHostFree(r.h_planes));
  r.h_planes = nullptr;
  r.h_cap    = 0;
  HIP_TRY(hipHostMalloc((void **)&r.h_planes, sizeof(double) * need, hipHostMallocDefault));
  r.h_cap = need;
  return 0;
}

// _read_begin once the mask (and form) have been checked: `need` doubles of planes, which launch(planes) writes on `st`
template <class Launch>
int read_begin(RDyHipOperator op, PlaneRead &r, int32_t comps, size_t need, const double *u_local, hipStream_t st, Launch launch) {
  if (op->n_owned == 0) {   // nothing is launched or copied: the read has landed as soon as it is waited for
    r.comps = comps;
    r.state = PlaneRead::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  int rc = read_reserve(op, r, need);
  if (rc) return rc;
  // an earlier read that has not landed is given up; its copy may still be reading the device planes, so this launch waits for it
  if (r.state == PlaneRead::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.done, 0));
  r.state = PlaneRead::NONE;
  rc = launch(r.d_planes.p);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(r.launched, st));
  HIP_TRY(hipStreamWaitEvent(op->stage.copy, r.launched, 0));
  HIP_TRY(hipMemcpyAsync(r.h_planes, r.d_planes.p, sizeof(double) * need, hipMemcpyDeviceToHost, op->stage.copy));
  HIP_TRY(hipEventRecord(r.done, op->stage.copy));
  r.comps = comps;
  r.state = PlaneRead::IN_FLIGHT;
  return 0;
}

int read_check_begun(const PlaneRead &r, OutputWords w) {
  if (r.state == PlaneRead::NONE) return fail(RDYHIP_ERR_USER, "no %sstate read has been begun (rdyhip_%sstate_read_begin)", w.noun, w.fn);
  return 0;
}

int read_ready(RDyHipOperator op, const PlaneRead &r, OutputWords w, int32_t *ready) {
  int rc = read_check_begun(r, w);
  if (rc) return rc;
  *ready = 1;
  if (r.state == PlaneRead::IN_FLIGHT && op->n_owned > 0) {
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

int read_wait(RDyHipOperator op, PlaneRead &r, OutputWords w) {
  int rc = read_check_begun(r, w);
  if (rc) return rc;
  if (r.state == PlaneRead::IN_FLIGHT && op->n_owned > 0) HIP_TRY(hipEventSynchronize(r.done));
  r.state = PlaneRead::LANDED;
  return 0;
}

// the state checks of _get and _ptr; *values = the pinned plane of (member, comp) among the planes of the last begin
int read_landed_plane(RDyHipOperator op, const PlaneRead &r, OutputWords w, int32_t member, int32_t comp, const double **values) {
  if (r.state != PlaneRead::LANDED) {
    int rc = read_check_begun(r, w);
    return rc ? rc : fail(RDYHIP_ERR_USER, "the %sstate read has not been waited for (rdyhip_%sstate_read_wait)", w.noun, w.fn);
  }
  if (!(r.comps & comp))
    return fail(RDYHIP_ERR_USER, "component 0x%x was not asked for by the last rdyhip_%sstate_read_begin (0x%x)", (unsigned)comp, w.fn, (unsigned)r.comps);
  const size_t plane = (size_t)member * (size_t)popcount(r.comps) + (size_t)popcount(r.comps & (comp - 1));
  *values = op->n_owned > 0 ? r.h_planes + plane * (size_t)op->n_owned : nullptr;
  return 0;
}

// _read_get once the member and the component have been checked
int read_get(RDyHipOperator op, const PlaneRead &r, OutputWords w, int32_t member, int32_t comp, int32_t size, double *values) {
  // CheckNumOwnedCells (src/rdydata.c:54-58)
  if (size != op->n_owned) return fail(RDYHIP_ERR_ARG_SIZ, "The size of array (%d) is not equal to the number of owned cells (%d)", size, op->n_owned);
  if (size > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  const double *plane = nullptr;
  int rc = read_landed_plane(op, r, w, member, comp, &plane);
  if (rc) return rc;
  if (size > 0) memcpy(values, plane, sizeof(double) * (size_t)size);
  return 0;
}

// ---- error sums ---------------------------------------------------------------------------------------------------------------

// the event, the pinned result of `width` doubles and the records of err_wg workgroups and the result, on the first call
int sums_reserve_records(SumsRead &s, int err_wg, size_t width) {
  if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  if (!s.h_sums) HIP_TRY(hipHostMalloc((void **)&s.h_sums, sizeof(double) * width, hipHostMallocDefault));
  if (s.d_records.p) return 0;
  DevBuf<double> records;
  int rc = records.alloc((size_t)(err_wg + 1) * width);
  if (!rc) s.d_records = std::move(records);
  return rc;
}

// areas by owned cell and the workgroup count, which all three states use, and the SWE state's own records, on the first error
// sums of any state (may synchronise)
int sums_reserve(RDyHipOperator op) {
  Readout &r = op->readout;
  if (r.d_area.p) return 0;
  const size_t no = (size_t)op->n_owned;
  std::vector<double> area(no);
  if (op->prefix) {
    std::copy(op->h_area.begin(), op->h_area.begin() + no, area.begin());
  } else {
    std::vector<int32_t> o2l(no);
    HIP_TRY(hipMemcpy(o2l.data(), op->d_o2l.p, sizeof(int32_t) * no, hipMemcpyDeviceToHost));
    for (size_t o = 0; o < no; ++o) area[o] = op->h_area[(size_t)o2l[o]];
  }
  const int wg = (int)std::min<int64_t>(((int64_t)op->n_owned + ERR_BLOCK - 1) / ERR_BLOCK, ERR_MAX_WG);
  DevBuf<double> d_area;
  int rc = d_area.upload(area);
  if (!rc) rc = sums_reserve_records(r.sums, wg, ERR_VALUES);
  if (rc) return rc;
  r.d_area = std::move(d_area);
  r.err_wg = wg;
  return 0;
}

// _error_sums once the operator (and feature) have been checked: launch(err_wg, records, result) on `st` leaves `width` doubles at
// `result`, which are copied to pinned memory behind it
template <class Launch>
int sums_begin(RDyHipOperator op, SumsRead &s, size_t width, const double *u_local, hipStream_t st, Launch launch) {
  if (op->n_owned == 0) {   // all zeros, nothing launched
    s.state = PlaneRead::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  int rc = sums_reserve(op);
  if (!rc) rc = sums_reserve_records(s, op->readout.err_wg, width);
  if (rc) return rc;
  // the records and the pinned result are shared by all calls: this one is ordered behind an earlier one that is still running
  if (s.state == PlaneRead::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, s.done, 0));
  double *result = s.d_records.p + (size_t)op->readout.err_wg * width;
  rc = launch(op->readout.err_wg, s.d_records.p, result);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(s.h_sums, result, sizeof(double) * width, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(s.done, st));
  s.state = PlaneRead::IN_FLIGHT;
  return 0;
}

// _error_sums_get: the sums have been asked for and, where anything was launched, have arrived in s.h_sums
int sums_wait(RDyHipOperator op, SumsRead &s, OutputWords w) {
  if (s.state == PlaneRead::NONE) return fail(RDYHIP_ERR_USER, "no %serror sums have been asked for (rdyhip_%serror_sums)", w.noun, w.fn);
  if (op->n_owned > 0 && s.state == PlaneRead::IN_FLIGHT) HIP_TRY(hipEventSynchronize(s.done));
  s.state = PlaneRead::LANDED;
  return 0;
}

// ---- output means -------------------------------------------------------------------------------------------------------------

// unknown bits, not exactly one variable: the argument errors the five calls share
int means_check_vars(int32_t vars, bool single) {
  if (vars & ~OUT_VARS) return fail(RDYHIP_ERR_USER, "unknown output variable bits 0x%x", (unsigned)(vars & ~OUT_VARS));
  if (single && vars != RDYHIP_OUTPUT_SOLUTION && vars != RDYHIP_OUTPUT_PRIMITIVE_VARIABLES && vars != RDYHIP_OUTPUT_SOURCES)
    return fail(RDYHIP_ERR_USER, "exactly one output variable is needed (got 0x%x)", (unsigned)vars);
  return 0;
}
int means_check_enabled(const OutputMeans &m, OutputWords w, int32_t vars) {
  for (int i = 0; i < 3; ++i)
    if ((vars >> i & 1) && !m.acc[i].p)
      return fail(RDYHIP_ERR_USER, "%soutput variable 0x%x is not enabled (rdyhip_%soutput_mean_enable)", w.noun, 1u << i, w.fn);
  return 0;
}

// zeroed accumulators of `doubles` values, with `members` times each, for the variables of `vars` that have none yet
int means_enable(OutputMeans &m, int32_t vars, size_t doubles, size_t members) {
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1) || m.acc[i].p) continue;   // an existing accumulator keeps its content
    DevBuf<double> a;
    int rc = a.zeros(doubles);
    if (rc) return rc;
    m.acc[i] = std::move(a);
    m.time[i].assign(members, 0.0);
  }
  return 0;
}

int means_reset(RDyHipOperator op, OutputMeans &m, int32_t vars, hipStream_t st) {
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1)) continue;
    if (op->n_owned > 0) HIP_TRY(hipMemsetAsync(m.acc[i].p, 0, m.acc[i].bytes(), st));
    std::fill(m.time[i].begin(), m.time[i].end(), 0.0);
  }
  return 0;
}

// _output_mean_time once the variable has been checked: one time per member
int means_time(const OutputMeans &m, OutputWords w, int32_t var, double *accumulated_times) {
  int rc = means_check_enabled(m, w, var);
  if (rc) return rc;
  const std::vector<double> &t = m.time[output_index(var)];
  std::copy(t.begin(), t.end(), accumulated_times);
  return 0;
}

// _output_mean_get of a state without members, once the variable has been checked: d_mean = acc / time over `width` values per cell
int means_get(RDyHipOperator op, const OutputMeans &m, OutputWords w, int32_t var, int width, double *d_mean, double *accumulated_time, hipStream_t st) {
  const double time = m.time[output_index(var)][0];
  if (op->n_owned > 0 && !d_mean) return fail(RDYHIP_ERR_USER, "null d_mean");
  // ComputeMean's PetscCheck (src/xdmf_output.c:213)
  if (!(time > 0.0)) return fail(RDYHIP_ERR_USER, "%soutput variable 0x%x: no time has been accumulated", w.noun, (unsigned)var);
  if (accumulated_time) *accumulated_time = time;
  const int64_t n = (int64_t)width * op->n_owned;
  if (n == 0) return 0;
  const double  s   = 1.0 / time;
  const double *acc = m.acc[output_index(var)].p;
  if (aligned16(acc) && aligned16(d_mean)) {
    const int64_t pairs = (n + 1) / 2;
    hipLaunchKernelGGL((output_mean_kernel<true>), dim3((unsigned)((pairs + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, st, n, s, acc, d_mean);
  } else {
    hipLaunchKernelGGL((output_mean_kernel<false>), dim3((unsigned)((n + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, st, n, s, acc, d_mean);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- observation series -------------------------------------------------------------------------------------------------------

// the argument checks of _series_enable after the operator's (and feature's), and the sites as local cells
int series_sites(RDyHipOperator op, const SeriesLog &s, OutputWords w, int32_t num_sites, const int32_t *owned_cell_ids, int32_t capacity,
                 std::vector<int32_t> &local) {
  if (num_sites < 0 || capacity < 0) return fail(RDYHIP_ERR_USER, "negative number of sites (%d) or capacity (%d)", num_sites, capacity);
  if (num_sites > 0 && !owned_cell_ids) return fail(RDYHIP_ERR_USER, "null owned_cell_ids");
  if (s.enabled) return fail(RDYHIP_ERR_USER, "the %sobservation series is enabled already", w.noun);
  for (int32_t i = 0; i < num_sites; ++i)
    if (owned_cell_ids[i] < 0 || owned_cell_ids[i] >= op->n_owned)
      return fail(RDYHIP_ERR_USER, "observation site %d: owned cell %d out of range [0, %d)", i, owned_cell_ids[i], op->n_owned);
  local.assign(owned_cell_ids, owned_cell_ids + num_sites);
  if (!op->prefix && num_sites > 0) {   // owned -> local through the operator's own table
    std::vector<int32_t> o2l((size_t)op->n_owned);
    HIP_TRY(hipMemcpy(o2l.data(), op->d_o2l.p, sizeof(int32_t) * (size_t)op->n_owned, hipMemcpyDeviceToHost));
    for (auto &c : local) c = o2l[(size_t)c];
  }
  return 0;
}

// the log of `capacity` records of `entries` rows of `width` doubles, with `members` times per record
int series_alloc_log(SeriesLog *s, int32_t entries, int32_t capacity, size_t width, size_t members = 1) {
  int rc = s->d_log.zeros((size_t)capacity * (size_t)entries * width);
  if (rc) return rc;
  s->entries  = entries;
  s->capacity = capacity;
  s->records  = 0;
  s->times.clear();
  s->times.reserve((size_t)capacity * members);
  s->enabled = true;
  return 0;
}

// an observation series of a feature: enabled, and with room for one more record
int series_check_enabled(const SeriesLog &s, OutputWords w) {
  if (!s.enabled) return fail(RDYHIP_ERR_USER, "the %sobservation series is not enabled (rdyhip_%sseries_enable)", w.noun, w.fn);
  return 0;
}
int series_check_room(const SeriesLog &s, OutputWords w) {
  if (s.records >= s.capacity)
    return fail(RDYHIP_ERR_USER, "%sseries: the log is full (%d records); read it and call rdyhip_%sseries_clear", w.noun, s.capacity, w.fn);
  return 0;
}

void series_info(const SeriesLog &s, int32_t *entries, int32_t *count, int32_t *capacity) {
  if (entries) *entries = s.entries;
  if (count) *count = s.records;
  if (capacity) *capacity = s.capacity;
}

void series_clear(SeriesLog &s) {
  s.times.clear();
  s.records = 0;
}

// records [first, first + count) of the series that messages call `name`: `members` times and `row` doubles per record
int series_read(const SeriesLog &s, const char *name, size_t row, size_t members, int32_t first, int32_t count, double *times, double *values,
                hipStream_t st) {
  if (first < 0 || count < 0 || (int64_t)first + count > (int64_t)s.records)
    return fail(RDYHIP_ERR_USER, "%s: records [%d, %d + %d) are not in the log (%d records)", name, first, first, count, s.records);
  if (count > 0 && (!times || (row > 0 && !values))) return fail(RDYHIP_ERR_USER, "null times / values");
  if (count == 0) return 0;
  std::copy(s.times.begin() + (size_t)first * members, s.times.begin() + ((size_t)first + (size_t)count) * members, times);
  if (row > 0) HIP_TRY(hipMemcpyAsync(values, s.d_log.p + (size_t)first * row, sizeof(double) * (size_t)count * row, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

}  // namespace
