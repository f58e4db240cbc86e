// Output of the [cell][3 + NT] tracer state on the device (rdyhip_tracer_state_*, rdyhip_tracer_error_sums,
// rdyhip_tracer_output_mean_*, rdyhip_tracer_series_*): what readout_kernels.h, output_kernels.h and series_kernels.h do for
// rows of three doubles, for rows of N = 3 + NT.  NT is a template argument of every kernel (1..7): rows and sums are
// per-thread arrays with compile-time indices and live in registers (a run-time width would put them in scratch).
//
//   planes, one lane per owned cell o, for the k-th set bit c_k of `comps` (ascending, 0 <= c_k < N):
//     planes[k][o] = row(loc(o))[c_k]
//   loc(o) = o where the owned cells are the first rows of the local vector, o2l[o] otherwise.  PRIM == false: row = the state's
//   row, moved as 64-bit integers -- nothing is computed, every bit pattern survives (-0.0, NaN payloads, denormals).
//   PRIM == true: row = (h, u, v, c_0 ...) by tracer_primitive_row below, which is the arithmetic of tracer_rhs_kernel's own
//   store of the primitive variables (tracer_kernels.h): h as it is, riemann_side(h, hu, hv, tiny_h, h_anuga_sq).u / .v,
//   tracer_concentrations<NT> (zero below tiny_h, the reciprocal taken once).  Only the components a plane or the arithmetic
//   needs are loaded (a row's components share its cache lines whichever of them are asked for); the stores of a wave are
//   contiguous 512-byte runs per plane.
//
//   error sums, e = u[loc(o)][c] - exact[o][c] (exact == nullptr: e = u), c < N: the scheme of error_partial_kernel /
//   error_finalize_kernel (readout_kernels.h) with records of 3 N + 1 values (l1[N], l2_squared[N], linf[N], area) instead of
//   ten: the same block size, the same number of workgroups G for n_owned, the same lane-to-cell assignment, the same fold
//   (err_fold<N> / err_block_fold_store<N> of readout_kernels.h, taken with N = 3 there: a shuffle tree over the lanes of a
//   wave, then the waves in order; in the second launch lane t takes records t, t + ERR_BLOCK, ...), and per component the same three operations.  Every order of addition depends on (n_owned, G) alone, so component c < 3
//   comes out as the bits error_partial_kernel gives for the [cell][3] slice of the same state.  At most 31 sums per lane, all in
//   registers.  (3 N + 1) * 8 bytes of LDS per wave, no scratch.
//
//   accumulate, one lane per owned cell, any subset of the three variables in one launch (a null accumulator leaves its variable out):
//     acc_s[o][c] = fma(dt, u_sol[loc(o)][c], acc_s[o][c])                       the solution
//     acc_p[o][c] = fma(dt, tracer_primitive_row(u_prim[loc(o)])[c], acc_p[o][c])  the primitive variables
//     acc_x[o][c] = fma(dt, c < 3 ? ext[o][c] : tsrc[o][c - 3], acc_x[o][c])     the sources: [owned][3] flow, [owned][NT] tracer
//   Where u_sol and u_prim are the same pointer the row is read once.  The fmas are written out.
//
//   observations, one lane per site s:  log[(r * S + s) * N + c] = u[site_local[s]][c]
//
// All four are pure streams with one lane per cell (site), the form the 3-wide kernels measured best for [cell][3] rows; with
// 32- to 80-byte rows a wave's N loads together cover whole lines while each instruction is strided.  No second form was built:
// the figures beside axpy_owned_kernel are profiles/tracer_output_ab.txt (RESULTS_LOG section 29).  Default cache policy
// throughout: the state is read again by the next RHS, the accumulators by the next step.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rdyhip.h"
#include "swe_device.h"
#include "readout_kernels.h"
#include "tracer_kernels.h"

namespace rdyhip {

constexpr int TOUT_BLOCK = 256;

// (h, u, v, c_0 ...) of one row (h, hu, hv, h c_0 ...): what tracer_rhs_kernel stores as primitive variables
template <int NT>
__device__ __forceinline__ void tracer_primitive_row(const double *row, double tiny_h, double h_anuga_sq, double *pv) {
  const RiemannSide p = riemann_side(row[0], row[1], row[2], tiny_h, h_anuga_sq);
  pv[0]               = row[0];
  pv[1]               = p.u;
  pv[2]               = p.v;
  tracer_concentrations<NT>(row[0], row + 3, tiny_h, pv + 3);
}

// One thread per owned cell; u and planes as 64-bit patterns.
template <int NT, bool PRIM>
__global__ void __launch_bounds__(TOUT_BLOCK) tracer_planes_kernel(int n_owned, const int32_t *__restrict__ o2l, int comps, double tiny_h,
                                                                    double h_anuga_sq, const uint64_t *__restrict__ u,
                                                                    uint64_t *__restrict__ planes) {
  constexpr int N = 3 + NT;
  const int64_t o = (int64_t)blockIdx.x * TOUT_BLOCK + threadIdx.x;
  if (o >= n_owned) return;
  const int64_t c = N * (o2l ? (int64_t)o2l[o] : o);
  uint64_t      row[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    row[k] = 0;
    if ((comps >> k & 1) || (PRIM && k == 0)) row[k] = u[c + k];   // every primitive variable needs h
  }
  if constexpr (PRIM) {
    double in[N], pv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) in[k] = __longlong_as_double((long long)row[k]);
    tracer_primitive_row<NT>(in, tiny_h, h_anuga_sq, pv);
#pragma unroll
    for (int k = 1; k < N; ++k) row[k] = (uint64_t)__double_as_longlong(pv[k]);   // h stays the pattern it was
  }
  uint64_t *p = planes + o;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (comps >> k & 1) {
      *p = row[k];
      p += n_owned;
    }
  }
}

// records[blockIdx.x][3 N + 1]: the sums over the owned cells o = blockIdx.x * ERR_BLOCK + threadIdx.x + j * gridDim.x * ERR_BLOCK
template <int NT>
__global__ void __launch_bounds__(ERR_BLOCK) tracer_error_partial_kernel(int n_owned, const int32_t *__restrict__ o2l, const double *__restrict__ u,
                                                                          const double *__restrict__ exact, const double *__restrict__ area,
                                                                          double *__restrict__ records) {
  constexpr int N = 3 + NT, V = 3 * N + 1;
  double        v[V];
#pragma unroll
  for (int i = 0; i < V; ++i) v[i] = 0.0;
  const int64_t step = (int64_t)gridDim.x * ERR_BLOCK;
  for (int64_t o = (int64_t)blockIdx.x * ERR_BLOCK + threadIdx.x; o < n_owned; o += step) {
    const int64_t c = N * (o2l ? (int64_t)o2l[o] : o);
    const double  a = area[o];
    double        e[N];
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = u[c + k];
    if (exact) {
#pragma unroll
      for (int k = 0; k < N; ++k) e[k] -= exact[N * o + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const double m = fabs(e[k]);
      v[k]         = fma(m, a, v[k]);
      v[N + k]     = fma(e[k] * e[k], a, v[N + k]);
      v[2 * N + k] = fmax(m, v[2 * N + k]);
    }
    v[3 * N] += a;
  }
  err_block_fold_store<N>(v, records + (int64_t)blockIdx.x * V);
}

// result[3 N + 1] = the fold of records[0 .. n_records); one workgroup
template <int NT>
__global__ void __launch_bounds__(ERR_BLOCK) tracer_error_finalize_kernel(int n_records, const double *__restrict__ records, double *__restrict__ result) {
  constexpr int N = 3 + NT, V = 3 * N + 1;
  double        v[V];
#pragma unroll
  for (int i = 0; i < V; ++i) v[i] = 0.0;
  for (int r = threadIdx.x; r < n_records; r += ERR_BLOCK) {
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = err_fold<N>(i, v[i], records[(int64_t)r * V + i]);
  }
  err_block_fold_store<N>(v, result);
}

// One thread per owned cell.
template <int NT>
__global__ void __launch_bounds__(TOUT_BLOCK) tracer_output_accumulate_kernel(int n_owned, const int32_t *__restrict__ o2l, double dt,
                                                                               const double *__restrict__ u_sol, double *__restrict__ acc_s,
                                                                               const double *__restrict__ u_prim, double tiny_h, double h_anuga_sq,
                                                                               double *__restrict__ acc_p, const double *__restrict__ ext,
                                                                               const double *__restrict__ tsrc, double *__restrict__ acc_x) {
  constexpr int N = 3 + NT;
  const int64_t o = (int64_t)blockIdx.x * TOUT_BLOCK + threadIdx.x;
  if (o >= n_owned) return;
  const int64_t c = N * (o2l ? (int64_t)o2l[o] : o);
  const int64_t r = N * o;
  double        up[N];
  if (acc_p) {
#pragma unroll
    for (int k = 0; k < N; ++k) up[k] = u_prim[c + k];
  }
  if (acc_s) {
    double us[N];
    if (acc_p && u_sol == u_prim) {
#pragma unroll
      for (int k = 0; k < N; ++k) us[k] = up[k];
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) us[k] = u_sol[c + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) acc_s[r + k] = fma(dt, us[k], acc_s[r + k]);
  }
  if (acc_p) {
    double pv[N];
    tracer_primitive_row<NT>(up, tiny_h, h_anuga_sq, pv);
#pragma unroll
    for (int k = 0; k < N; ++k) acc_p[r + k] = fma(dt, pv[k], acc_p[r + k]);
  }
  if (acc_x) {
    double x[N];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = ext[3 * o + k];
#pragma unroll
    for (int j = 0; j < NT; ++j) x[3 + j] = tsrc[NT * o + j];
#pragma unroll
    for (int k = 0; k < N; ++k) acc_x[r + k] = fma(dt, x[k], acc_x[r + k]);
  }
}

// One thread per site.
template <int NT>
__global__ void tracer_series_observe_kernel(int S, const int32_t *__restrict__ site_local, const double *__restrict__ u, int64_t r,
                                             double *__restrict__ dlog) {
  constexpr int N = 3 + NT;
  const int     s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int64_t c   = N * (int64_t)site_local[s];
  const int64_t row = (r * S + s) * N;
  double        v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = u[c + k];
#pragma unroll
  for (int k = 0; k < N; ++k) dlog[row + k] = v[k];
}

}  // namespace rdyhip
