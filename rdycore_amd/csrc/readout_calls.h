// State read-out behind the C ABI (rdyhip_state_planes, rdyhip_state_read_*, rdyhip_error_sums*; kernels: readout_kernels.h):
// the owned-cell getters through pinned planes and the error sums, over output_shared.h.  Included by rdyhip_api.hip only.
#pragma once
namespace {

constexpr int32_t READ_COMPS = RDYHIP_COMPONENT_H | RDYHIP_COMPONENT_HU | RDYHIP_COMPONENT_HV;

bool one_component(int32_t comp) { return comp == RDYHIP_COMPONENT_H || comp == RDYHIP_COMPONENT_HU || comp == RDYHIP_COMPONENT_HV; }

int launch_state_planes(RDyHipOperator op, int32_t comps, const double *u, double *planes, hipStream_t st) {
  hipLaunchKernelGGL(state_planes_kernel, dim3((unsigned)((op->n_owned + READ_BLOCK - 1) / READ_BLOCK)), dim3(READ_BLOCK), 0, st, op->n_owned,
                     owned_to_local(op), (int)comps, (const uint64_t *)u, (uint64_t *)planes);
  HIP_TRY(hipGetLastError());
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
  hipStream_t st = (hipStream_t)stream;
  return read_begin(op, op->readout.planes, comps, (size_t)popcount(comps) * (size_t)op->n_owned, u_local, st,
                    [&](double *planes) { return launch_state_planes(op, comps, u_local, planes, st); });
}

extern "C" int rdyhip_state_read_ready(RDyHipOperator op, int32_t *ready) {
  if (!op || !ready) return fail(RDYHIP_ERR_USER, "null argument");
  return read_ready(op, op->readout.planes, SWE_WORDS, ready);
}

extern "C" int rdyhip_state_read_wait(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  return read_wait(op, op->readout.planes, SWE_WORDS);
}

extern "C" int rdyhip_state_read_get(RDyHipOperator op, int32_t comp, int32_t size, double *values) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (!one_component(comp)) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comp);
  return read_get(op, op->readout.planes, SWE_WORDS, 0, comp, size, values);
}

extern "C" int rdyhip_state_read_ptr(RDyHipOperator op, int32_t comp, const double **pinned_values) {
  if (!op || !pinned_values) return fail(RDYHIP_ERR_USER, "null argument");
  if (!one_component(comp)) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comp);
  return read_landed_plane(op, op->readout.planes, SWE_WORDS, 0, comp, pinned_values);
}

extern "C" int rdyhip_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  hipStream_t st = (hipStream_t)stream;
  return sums_begin(op, op->readout.sums, ERR_VALUES, u_local, st, [&](int wg, double *records, double *result) {
    hipLaunchKernelGGL(error_partial_kernel, dim3(wg), dim3(ERR_BLOCK), 0, st, op->n_owned, owned_to_local(op), u_local, d_exact, op->readout.d_area.p,
                       records);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(error_finalize_kernel, dim3(1), dim3(ERR_BLOCK), 0, st, wg, records, result);
    HIP_TRY(hipGetLastError());
    return 0;
  });
}

extern "C" int rdyhip_error_sums_get(RDyHipOperator op, RDyHipErrorSums *out) {
  if (!op || !out) return fail(RDYHIP_ERR_USER, "null argument");
  int rc = sums_wait(op, op->readout.sums, SWE_WORDS);
  if (rc) return rc;
  static_assert(sizeof(RDyHipErrorSums) == sizeof(double) * ERR_VALUES, "RDyHipErrorSums is the ten doubles of a record");
  if (op->n_owned == 0) {
    memset(out, 0, sizeof(*out));
  } else {
    memcpy(out, op->readout.sums.h_sums, sizeof(*out));
  }
  return 0;
}
