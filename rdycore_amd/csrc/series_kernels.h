// The time series of WriteTimeSeries (src/time_series.c:530-564) kept on the device (rdyhip_series_*): one launch per record,
// appended to a log that stays in device memory until the host reads it.
//
//   boundary fluxes, one lane per boundary edge k of the operator (all boundaries concatenated, the rows of boundary_fluxes_accum):
//     if slot[k] >= 0:  log[(r * E + slot[k]) * 3 + c] = (len[k] * acc[k][c]) / T      c = 0..2
//     acc[k][c] = +0.0                                                                  every k, recorded or not
//   RecordBoundaryFluxes' edge_len * value (287-289) and WriteBoundaryFluxes' / accumulated_time (325-327) are two roundings
//   in the reference and two here: a product, then a division by T -- never a multiplication by 1 / T.  T is the accumulated
//   time, or 1.0 where that is exactly 0 (311-313; decided on the host).  A NaN accumulator (an edge dry on both sides) is a
//   NaN in the record.  The reset is ResetAccumulatedBoundaryFluxes' VecZeroEntries of every boundary (520-523), the
//   unlisted ones and the edges behind ghost cells included.
//
//   observations, one lane per site s:
//     log[(r * S + s) * 3 + c] = u_local[site_local[s]][c]                              the VecCopy at 541 + the scatter of 399-402
//
// r is the record number, E / S the rows of a record.  K and S are thousands at most: the kernels are a few workgroups of
// plain loads and stores with the default cache policy, no LDS, no scratch.  They exist so that the step loop needs no host
// synchronisation to keep a series.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rdyhip {

constexpr int SERIES_BLOCK = 256;

__global__ void series_boundary_record_kernel(int K, const int32_t *__restrict__ slot, const double *__restrict__ len, double T, int64_t r,
                                              int64_t E, double *__restrict__ acc, double *__restrict__ dlog) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int64_t a  = 3 * (int64_t)k;
  const double  a0 = acc[a + 0], a1 = acc[a + 1], a2 = acc[a + 2];
  const int32_t s  = slot[k];
  if (s >= 0) {
    const double  l   = len[k];
    const int64_t row = (r * E + s) * 3;
    dlog[row + 0]      = (l * a0) / T;
    dlog[row + 1]      = (l * a1) / T;
    dlog[row + 2]      = (l * a2) / T;
  }
  acc[a + 0] = 0.0;
  acc[a + 1] = 0.0;
  acc[a + 2] = 0.0;
}

__global__ void series_observe_kernel(int S, const int32_t *__restrict__ site_local, const double *__restrict__ u_local, int64_t r,
                                      double *__restrict__ dlog) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int64_t c   = 3 * (int64_t)site_local[s];
  const int64_t row = (r * S + s) * 3;
  dlog[row + 0]      = u_local[c + 0];
  dlog[row + 1]      = u_local[c + 1];
  dlog[row + 2]      = u_local[c + 2];
}

}  // namespace rdyhip
