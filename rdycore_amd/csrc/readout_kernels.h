// Reading the state out on the device (rdyhip_state_planes, rdyhip_state_read_*, rdyhip_error_sums): the owned-cell getters
// RDyGetOwnedCell{Heights,XMomenta,YMomenta} (src/rdydata.c:171-205) and the rank-local loops of RDyMMSComputeErrorNorms
// (src/rdymms.c:869-880) without the copy of the whole [cell][3] state to the host.
//
//   planes, one lane per owned cell o, for the k-th set bit c_k of `comps` (ascending):
//     planes[k][o] = u_local[loc(o)][c_k]
//   loc(o) = o where the owned cells are the first rows of the local vector, o2l[o] otherwise (as output_kernels.h).  The values
//   are moved as 64-bit integers: nothing is computed, every bit pattern survives (-0.0, NaN payloads, denormals).
//   A pure stream, 24 B read per cell (a row's three components share its cache lines whichever of them is asked for) and 8 B
//   written per component.  A lane takes a cell, the form output_kernels.h found best for [cell][3] rows; the stores of a wave
//   are contiguous 512-byte runs.  Default cache policy: the state is read again by the next RHS launch.  No LDS, no scratch.
//   Measured (profiles/readout_ab.txt, RESULTS_LOG section 20): at 10 M cells 0.42 x axpy_owned_kernel's time for one component
//   and 0.67 x for three, on the byte ratios (24 + 8 k) / 72 = 0.44 and 0.67; no other form was built.
//
//   error sums, e = u_local[loc(o)][c] - exact[o][c] (one subtraction, VecAYPX at src/rdymms.c:857; exact == nullptr: e = u):
//     l1[c]  = sum_o fma(|e|, area[o], .)      l2_squared[c] = sum_o fma(e * e, area[o], .)
//     linf[c] = max_o |e|                       area = sum_o area[o]
//   Two launches and no atomics, the pattern of the Courant buckets and courant_finalize_kernel (swe_kernels.h):
//   error_partial_kernel -- G workgroups of ERR_BLOCK lanes walk the owned cells with a stride of G * ERR_BLOCK, every lane keeps
//   its ten sums in registers, the workgroup folds them (lanes of a wave by shuffles in a fixed tree, the waves through LDS in
//   wave order) and stores one record of ten doubles; error_finalize_kernel -- one workgroup folds the G records the same way,
//   lane t taking records t, t + ERR_BLOCK, ... in that order.  Which lane sees which cell and every order of addition depend
//   on (n_owned, G) alone, and G on n_owned alone: the result is the same bits on every run and every stream.  The sums are
//   fused multiply-adds, written out.  NaN: a NaN e makes l1 and l2_squared of its component NaN; linf is formed with fmax,
//   which drops a NaN operand (the reference's PetscMax is order-dependent there; rdyhip.h leaves it unspecified).
//   80 bytes of LDS per wave in each of the two kernels, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rdyhip.h"

namespace rdyhip {

constexpr int READ_BLOCK  = 256;
constexpr int ERR_BLOCK   = RDYHIP_ERROR_SUMS_BLOCK;
constexpr int ERR_MAX_WG  = RDYHIP_ERROR_SUMS_MAX_WORKGROUPS;
constexpr int ERR_VALUES  = 10;   // l1[3], l2_squared[3], linf[3], area: RDyHipErrorSums
constexpr int ERR_WAVES   = ERR_BLOCK / 64;

// One thread per owned cell; u and planes as 64-bit patterns.
__global__ void state_planes_kernel(int n_owned, const int32_t *__restrict__ o2l, int comps, const uint64_t *__restrict__ u,
                                    uint64_t *__restrict__ planes) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_owned) return;
  const int64_t c = 3 * (o2l ? (int64_t)o2l[o] : o);
  uint64_t      v0 = 0, v1 = 0, v2 = 0;
  if (comps & 1) v0 = u[c + 0];
  if (comps & 2) v1 = u[c + 1];
  if (comps & 4) v2 = u[c + 2];
  uint64_t *p = planes + o;
  if (comps & 1) {
    *p = v0;
    p += n_owned;
  }
  if (comps & 2) {
    *p = v1;
    p += n_owned;
  }
  if (comps & 4) *p = v2;
}

// A record of 3 N + 1 values (N = 3: the SWE and ensemble records of ERR_VALUES; tracers: N = 3 + NT): values [2 N, 3 N) are
// maxima, the others sums
template <int N>
__device__ __forceinline__ double err_fold(int i, double a, double b) {
  return (i >= 2 * N && i < 3 * N) ? fmax(a, b) : a + b;
}

// The workgroup's fold of v[3 N + 1]: lanes of a wave by a shuffle tree, then the waves in order; thread 0 stores the record.
template <int N>
__device__ __forceinline__ void err_block_fold_store(double (&v)[3 * N + 1], double *__restrict__ record) {
  constexpr int   V = 3 * N + 1;
  __shared__ double waves[ERR_WAVES][V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v[i] = err_fold<N>(i, v[i], __shfl_down(v[i], d, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) waves[wave][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      double r = waves[0][i];
#pragma unroll
      for (int w = 1; w < ERR_WAVES; ++w) r = err_fold<N>(i, r, waves[w][i]);
      record[i] = r;
    }
  }
}

// records[blockIdx.x][ERR_VALUES]: the sums over the owned cells o = blockIdx.x * ERR_BLOCK + threadIdx.x + j * gridDim.x * ERR_BLOCK
__global__ void __launch_bounds__(ERR_BLOCK) error_partial_kernel(int n_owned, const int32_t *__restrict__ o2l, const double *__restrict__ u,
                                                                   const double *__restrict__ exact, const double *__restrict__ area,
                                                                   double *__restrict__ records) {
  double v[ERR_VALUES];
#pragma unroll
  for (int i = 0; i < ERR_VALUES; ++i) v[i] = 0.0;
  const int64_t step = (int64_t)gridDim.x * ERR_BLOCK;
  for (int64_t o = (int64_t)blockIdx.x * ERR_BLOCK + threadIdx.x; o < n_owned; o += step) {
    const int64_t c = 3 * (o2l ? (int64_t)o2l[o] : o);
    const double  a = area[o];
    double        e[3] = {u[c + 0], u[c + 1], u[c + 2]};
    if (exact) {
      e[0] -= exact[3 * o + 0];
      e[1] -= exact[3 * o + 1];
      e[2] -= exact[3 * o + 2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double m = fabs(e[k]);
      v[k]     = fma(m, a, v[k]);
      v[3 + k] = fma(e[k] * e[k], a, v[3 + k]);
      v[6 + k] = fmax(m, v[6 + k]);
    }
    v[9] += a;
  }
  err_block_fold_store<3>(v, records + (int64_t)blockIdx.x * ERR_VALUES);
}

// result[ERR_VALUES] = the fold of records[0 .. n_records); one workgroup
__global__ void __launch_bounds__(ERR_BLOCK) error_finalize_kernel(int n_records, const double *__restrict__ records, double *__restrict__ result) {
  double v[ERR_VALUES];
#pragma unroll
  for (int i = 0; i < ERR_VALUES; ++i) v[i] = 0.0;
  for (int r = threadIdx.x; r < n_records; r += ERR_BLOCK) {
#pragma unroll
    for (int i = 0; i < ERR_VALUES; ++i) v[i] = err_fold<3>(i, v[i], records[(int64_t)r * ERR_VALUES + i]);
  }
  err_block_fold_store<3>(v, result);
}

}  // namespace rdyhip
