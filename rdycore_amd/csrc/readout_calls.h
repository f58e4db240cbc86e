// State read-out behind the C ABI (rdyhip_state_planes, rdyhip_state_read_*, rdyhip_error_sums*; kernels: readout_kernels.h):
// the owned-cell getters through pinned planes and the error sums.  Included by rdyhip_api.hip only.
#pragma once
namespace {

constexpr int32_t READ_COMPS = RDYHIP_COMPONENT_H | RDYHIP_COMPONENT_HU | RDYHIP_COMPONENT_HV;

int popcount3(int32_t comps) { return (comps & 1) + (comps >> 1 & 1) + (comps >> 2 & 1); }
bool one_component(int32_t comp) { return comp == RDYHIP_COMPONENT_H || comp == RDYHIP_COMPONENT_HU || comp == RDYHIP_COMPONENT_HV; }

int launch_state_planes(RDyHipOperator op, int32_t comps, const double *u, double *planes, hipStream_t st) {
  hipLaunchKernelGGL(state_planes_kernel, dim3((unsigned)((op->n_owned + READ_BLOCK - 1) / READ_BLOCK)), dim3(READ_BLOCK), 0, st, op->n_owned,
                     op->prefix ? (const int32_t *)nullptr : op->d_o2l.p, (int)comps, (const uint64_t *)u, (uint64_t *)planes);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the copy stream (shared with the setters' staging ring), the two events, and room for `k` planes on the device and in pinned
// memory: grows only; a call that allocates may synchronise, and waits first for a copy that still reads the old buffers
int read_reserve(RDyHipOperator op, int k) {
  Readout &r = op->readout;
  if (!op->stage.copy) HIP_TRY(hipStreamCreateWithFlags(&op->stage.copy, hipStreamNonBlocking));
  if (!r.launched) HIP_TRY(hipEventCreateWithFlags(&r.launched, hipEventDisableTiming));
  if (!r.done) HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  const size_t need = (size_t)k * (size_t)op->n_owned;
  if (r.d_planes.p && r.d_planes.n >= need && r.h_cap >= need) return 0;
  if (r.state == Readout::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.done));
  r.state = Readout::NONE;   // whatever had been read lived in the old buffers
  int rc = r.d_planes.alloc(need);
  if (rc) return rc;
  if (r.h_planes) HIP_TRY(hipHostFree(r.h_planes));
  r.h_planes = nullptr;
  r.h_cap    = 0;
  HIP_TRY(hipHostMalloc((void **)&r.h_planes, sizeof(double) * need, hipHostMallocDefault));
  r.h_cap = need;
  return 0;
}

// the arguments of _get and _ptr; *plane = the index of `comp` among the planes of the last begin
int read_check_landed(RDyHipOperator op, int32_t comp, int *plane) {
  const Readout &r = op->readout;
  if (r.state != Readout::LANDED)
    return fail(RDYHIP_ERR_USER, r.state == Readout::NONE ? "no state read has been begun (rdyhip_state_read_begin)"
                                                          : "the state read has not been waited for (rdyhip_state_read_wait)");
  if (!(r.comps & comp)) return fail(RDYHIP_ERR_USER, "component 0x%x was not asked for by the last rdyhip_state_read_begin (0x%x)", (unsigned)comp, (unsigned)r.comps);
  *plane = popcount3(r.comps & (comp - 1));
  return 0;
}

// areas by owned cell, the partial records and the pinned result of the error sums, on the first call (may synchronise)
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
  if (!r.sums_done) HIP_TRY(hipEventCreateWithFlags(&r.sums_done, hipEventDisableTiming));
  if (!r.h_sums) HIP_TRY(hipHostMalloc((void **)&r.h_sums, sizeof(double) * ERR_VALUES, hipHostMallocDefault));
  DevBuf<double> records, d_area;
  int rc = records.alloc((size_t)(wg + 1) * ERR_VALUES);
  if (!rc) rc = d_area.upload(area);
  if (rc) return rc;
  r.d_records = std::move(records);
  r.d_area    = std::move(d_area);
  r.err_wg    = wg;
  return 0;
}

}  // namespace

extern "C" int rdyhip_state_planes(RDyHipOperator op, int32_t comps, const double *u_local, double *d_planes, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (comps < 1 || comps > READ_COMPS) return fail(RDYHIP_ERR_USER, "component mask 0x%x is not in 1..7 (RDYHIP_COMPONENT_*)", (unsigned)comps);
  if (op->n_owned == 0) return 0;
  if (!u_local || !d_planes) return fail(RDYHIP_ERR_USER, "null u_local / d_planes");
  return launch_state_planes(op, comps, u_local, d_planes, (hipStream_t)stream);
}

extern "C" int rdyhip_state_read_begin(RDyHipOperator op, int32_t comps, const double *u_local, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (comps < 1 || comps > READ_COMPS) return fail(RDYHIP_ERR_USER, "component mask 0x%x is not in 1..7 (RDYHIP_COMPONENT_*)", (unsigned)comps);
  Readout &r = op->readout;
  if (op->n_owned == 0) {   // nothing is launched or copied: the read has landed as soon as it is waited for
    r.comps = comps;
    r.state = Readout::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  hipStream_t st = (hipStream_t)stream;
  const int   k  = popcount3(comps);
  int rc = read_reserve(op, k);
  if (rc) return rc;
  // an earlier read that has not landed is given up; its copy may still be reading the device planes, so this launch waits for it
  if (r.state == Readout::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.done, 0));
  r.state = Readout::NONE;
  rc = launch_state_planes(op, comps, u_local, r.d_planes.p, st);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(r.launched, st));
  HIP_TRY(hipStreamWaitEvent(op->stage.copy, r.launched, 0));
  HIP_TRY(hipMemcpyAsync(r.h_planes, r.d_planes.p, sizeof(double) * (size_t)k * (size_t)op->n_owned, hipMemcpyDeviceToHost, op->stage.copy));
  HIP_TRY(hipEventRecord(r.done, op->stage.copy));
  r.comps = comps;
  r.state = Readout::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_state_read_ready(RDyHipOperator op, int32_t *ready) {
  if (!op || !ready) return fail(RDYHIP_ERR_USER, "null argument");
  const Readout &r = op->readout;
  if (r.state == Readout::NONE) return fail(RDYHIP_ERR_USER, "no state read has been begun (rdyhip_state_read_begin)");
  *ready = 1;
  if (r.state == Readout::IN_FLIGHT && op->n_owned > 0) {
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

extern "C" int rdyhip_state_read_wait(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  Readout &r = op->readout;
  if (r.state == Readout::NONE) return fail(RDYHIP_ERR_USER, "no state read has been begun (rdyhip_state_read_begin)");
  if (r.state == Readout::IN_FLIGHT && op->n_owned > 0) HIP_TRY(hipEventSynchronize(r.done));
  r.state = Readout::LANDED;
  return 0;
}

extern "C" int rdyhip_state_read_get(RDyHipOperator op, int32_t comp, int32_t size, double *values) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (!one_component(comp)) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comp);
  // CheckNumOwnedCells (src/rdydata.c:54-58)
  if (size != op->n_owned) return fail(RDYHIP_ERR_ARG_SIZ, "The size of array (%d) is not equal to the number of owned cells (%d)", size, op->n_owned);
  if (size > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  int plane = 0;
  int rc = read_check_landed(op, comp, &plane);
  if (rc) return rc;
  if (size > 0) memcpy(values, op->readout.h_planes + (size_t)plane * (size_t)op->n_owned, sizeof(double) * (size_t)size);
  return 0;
}

extern "C" int rdyhip_state_read_ptr(RDyHipOperator op, int32_t comp, const double **pinned_values) {
  if (!op || !pinned_values) return fail(RDYHIP_ERR_USER, "null argument");
  if (!one_component(comp)) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comp);
  int plane = 0;
  int rc = read_check_landed(op, comp, &plane);
  if (rc) return rc;
  *pinned_values = op->n_owned > 0 ? op->readout.h_planes + (size_t)plane * (size_t)op->n_owned : nullptr;
  return 0;
}

extern "C" int rdyhip_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  Readout &r = op->readout;
  if (op->n_owned == 0) {   // all zeros, nothing launched
    r.sums_state = Readout::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  int rc = sums_reserve(op);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the records and the pinned result are shared by all calls: this one is ordered behind an earlier one that is still running
  if (r.sums_state == Readout::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.sums_done, 0));
  double *result = r.d_records.p + (size_t)r.err_wg * ERR_VALUES;
  hipLaunchKernelGGL(error_partial_kernel, dim3(r.err_wg), dim3(ERR_BLOCK), 0, st, op->n_owned, op->prefix ? (const int32_t *)nullptr : op->d_o2l.p,
                     u_local, d_exact, r.d_area.p, r.d_records.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(error_finalize_kernel, dim3(1), dim3(ERR_BLOCK), 0, st, r.err_wg, r.d_records.p, result);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(r.h_sums, result, sizeof(double) * ERR_VALUES, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(r.sums_done, st));
  r.sums_state = Readout::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_error_sums_get(RDyHipOperator op, RDyHipErrorSums *out) {
  if (!op || !out) return fail(RDYHIP_ERR_USER, "null argument");
  Readout &r = op->readout;
  if (r.sums_state == Readout::NONE) return fail(RDYHIP_ERR_USER, "no error sums have been asked for (rdyhip_error_sums)");
  static_assert(sizeof(RDyHipErrorSums) == sizeof(double) * ERR_VALUES, "RDyHipErrorSums is the ten doubles of a record");
  if (op->n_owned == 0) {
    memset(out, 0, sizeof(*out));
  } else {
    if (r.sums_state == Readout::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.sums_done));
    memcpy(out, r.h_sums, sizeof(*out));
  }
  r.sums_state = Readout::LANDED;
  return 0;
}

