// Output of the [B][cell][3] ensemble state on the device (rdyhip_ens_state_*, rdyhip_ens_error_sums, rdyhip_ens_output_mean_*,
// rdyhip_ens_series_*, rdyhip_ens_stats): what readout_kernels.h, output_kernels.h and series_kernels.h do for one [cell][3]
// state, for all B members in one launch, and the per-cell statistics over the members.  Member m's state is the slice
// u + m * u_stride (u_stride = 3 num_cells), as ensemble_kernels.h takes it.
//
//   planes, one lane per (owned cell o, member m), for the k-th set bit c_k of `comps` (ascending), K = popcount(comps):
//     planes[(m * K + k) * n_owned + o] = u[m][loc(o)][c_k]
//   loc(o) = o where the owned cells are the first rows of the local vector, o2l[o] otherwise.  Values move as 64-bit integers:
//   nothing is computed, every bit pattern survives (-0.0, NaN payloads, denormals).  Member m's planes are what
//   state_planes_kernel writes for member m's slice.
//
//   error sums, e = u[m][loc(o)][c] - exact[m][o][c] (exact == nullptr: e = u): error_partial_kernel / error_finalize_kernel
//   (readout_kernels.h) with blockIdx.y = member in the first launch and blockIdx.x = member in the second: the same block size,
//   the same G workgroups per member for n_owned, the same lane-to-cell assignment, the same three operations per component, and
//   the folds are readout_kernels.h's own device functions (err_fold, err_block_fold_store).  Every order of addition depends on
//   (n_owned, G) alone: member m's record is the bits error_partial_kernel + error_finalize_kernel give for member m's slice.
//   records [B][G][10], results [B][10].  80 bytes of LDS per wave, no atomics, no scratch.
//
//   accumulate, one lane per (owned cell, member), any subset of the three variables (a null accumulator leaves its variable out):
//   out_accumulate_cell of output_kernels.h -- the very function output_accumulate_kernel runs, in its "derive" form (no stored
//   primitive variables) -- on member m's slices with dt = dts[m]:
//     acc_s[m][o] = fma(dts[m], u_sol[m][loc(o)], acc_s[m][o])
//     acc_p[m][o] = fma(dts[m], (h, u, v) of riemann_side(u_prim[m][loc(o)]), acc_p[m][o])
//     acc_x[m][o] = fma(dts[m], ext[m][o], acc_x[m][o])          ext: the members' own source [B][owned][3]
//   Where u_sol == u_prim the row is read once.  mean: mean[m][i] = acc[m][i] * s[m], s[m] = 1 / accumulated time of member m,
//   formed on the host (output_mean_kernel's product, one scale per member).
//
//   observations, one lane per (site s, member m):  log[((r * B + m) * S + s) * 3 + c] = u[m][site_local[s]][c]
//
//   statistics over the members, one lane per owned cell o; the lane loads loc(o) once and walks the members as the RHS kernel
//   walks them with its geometry.  For the k-th set bit c_k of `comps` and x_m = u[m][loc(o)][c_k]:
//     stats[(3 k + 0) * n_owned + o] = (((x_0 + x_1) + x_2) + ... + x_{B-1}) * (1.0 / B)     mean: adds in member order, one product
//     stats[(3 k + 1) * n_owned + o] = r, r = x_0; r = (x_m < r) ? x_m : r                    min, in member order
//     stats[(3 k + 2) * n_owned + o] = r, r = x_0; r = (x_m > r) ? x_m : r                    max, in member order
//   Comparisons, not fmin / fmax: of equal values (+0.0 and -0.0 included) the earlier member's bits stay; a NaN in a later
//   member never replaces the running value (both comparisons are false); a NaN in member 0 stays to the end, for the same
//   reason.  The mean's NaN is the sum's.  Each lane reads its 24-byte row of every member, u_stride apart, and a wave stores
//   contiguous 512-byte runs per plane.
//
// The launch shape: planes, partial sums, accumulate and observations take the member from the grid ((blocks, B)), not from a
// loop in the lane.  They are pure streams with nothing to share between the members but loc(o) -- 4 of the 28 to 148 bytes a lane
// moves, and o2l is L2-resident across the B workgroups that read the same entries -- while a member loop would cut the number of
// workgroups by B: on the meshes ensembles are run on (tens of thousands of cells) a one-member grid leaves most of the 256 CUs
// without a wave, and the grid form fills them from B = 2 on.  The statistics are the one kernel whose lane needs every member,
// so there the lane walks.  Figures: profiles/ens_output_ab.txt.  Default cache policy throughout: the state is read again by
// the next evaluation, the accumulators by the next step.  No floating-point atomics; results are the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rdyhip.h"
#include "output_kernels.h"
#include "readout_kernels.h"

namespace rdyhip {

constexpr int ENS_OUT_BLOCK = 256;

// one value per member, by value in the kernel arguments (as EnsembleArgs::dts)
struct EnsPerMember {
  double v[RDYHIP_MAX_ENSEMBLE_MEMBERS];
};

// blockIdx.y: the member.  u and planes as 64-bit patterns; n_planes = popcount(comps).
__global__ void __launch_bounds__(ENS_OUT_BLOCK) ens_planes_kernel(int n_owned, const int32_t *__restrict__ o2l, int comps, int n_planes, int64_t u_stride,
                                                                   const uint64_t *__restrict__ u, uint64_t *__restrict__ planes) {
  const int64_t o = (int64_t)blockIdx.x * ENS_OUT_BLOCK + threadIdx.x;
  if (o >= n_owned) return;
  const int64_t   m  = blockIdx.y;
  const uint64_t *um = u + m * u_stride + 3 * (o2l ? (int64_t)o2l[o] : o);
  uint64_t        v0 = 0, v1 = 0, v2 = 0;
  if (comps & 1) v0 = um[0];
  if (comps & 2) v1 = um[1];
  if (comps & 4) v2 = um[2];
  uint64_t *p = planes + m * n_planes * (int64_t)n_owned + o;
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

// records[blockIdx.y][blockIdx.x][ERR_VALUES]: error_partial_kernel's sums for member blockIdx.y
__global__ void __launch_bounds__(ERR_BLOCK) ens_error_partial_kernel(int n_owned, const int32_t *__restrict__ o2l, int64_t u_stride,
                                                                      const double *__restrict__ u, const double *__restrict__ exact,
                                                                      const double *__restrict__ area, double *__restrict__ records) {
  const int64_t m  = blockIdx.y;
  const double *um = u + m * u_stride;
  const double *xm = exact ? exact + m * 3 * (int64_t)n_owned : nullptr;
  double        v[ERR_VALUES];
#pragma unroll
  for (int i = 0; i < ERR_VALUES; ++i) v[i] = 0.0;
  const int64_t step = (int64_t)gridDim.x * ERR_BLOCK;
  for (int64_t o = (int64_t)blockIdx.x * ERR_BLOCK + threadIdx.x; o < n_owned; o += step) {
    const int64_t c = 3 * (o2l ? (int64_t)o2l[o] : o);
    const double  a = area[o];
    double        e[3] = {um[c + 0], um[c + 1], um[c + 2]};
    if (xm) {
      e[0] -= xm[3 * o + 0];
      e[1] -= xm[3 * o + 1];
      e[2] -= xm[3 * o + 2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double q = fabs(e[k]);
      v[k]     = fma(q, a, v[k]);
      v[3 + k] = fma(e[k] * e[k], a, v[3 + k]);
      v[6 + k] = fmax(q, v[6 + k]);
    }
    v[9] += a;
  }
  err_block_fold_store<3>(v, records + (m * gridDim.x + blockIdx.x) * ERR_VALUES);
}

// results[blockIdx.x][ERR_VALUES] = the fold of records[blockIdx.x][0 .. n_records); workgroup m for member m
__global__ void __launch_bounds__(ERR_BLOCK) ens_error_finalize_kernel(int n_records, const double *__restrict__ records, double *__restrict__ results) {
  const double *rm = records + (int64_t)blockIdx.x * n_records * ERR_VALUES;
  double        v[ERR_VALUES];
#pragma unroll
  for (int i = 0; i < ERR_VALUES; ++i) v[i] = 0.0;
  for (int r = threadIdx.x; r < n_records; r += ERR_BLOCK) {
#pragma unroll
    for (int i = 0; i < ERR_VALUES; ++i) v[i] = err_fold<3>(i, v[i], rm[(int64_t)r * ERR_VALUES + i]);
  }
  err_block_fold_store<3>(v, results + (int64_t)blockIdx.x * ERR_VALUES);
}

// blockIdx.y: the member.  Accumulators and ext are [B][n_owned][3]; a null pointer leaves its variable out.
__global__ void __launch_bounds__(ENS_OUT_BLOCK) ens_output_accumulate_kernel(int n_owned, const int32_t *__restrict__ o2l, const EnsPerMember dts,
                                                                              int64_t u_stride, const double *__restrict__ u_sol,
                                                                              double *__restrict__ acc_s, const double *__restrict__ u_prim,
                                                                              double tiny_h, double h_anuga_sq, double *__restrict__ acc_p,
                                                                              const double *__restrict__ ext, double *__restrict__ acc_x) {
  const int64_t o = (int64_t)blockIdx.x * ENS_OUT_BLOCK + threadIdx.x;
  if (o >= n_owned) return;
  const int64_t m = blockIdx.y, us = m * u_stride, as = m * 3 * (int64_t)n_owned;
  out_accumulate_cell(o, o2l ? (int64_t)o2l[o] : o, dts.v[m], u_sol ? u_sol + us : nullptr, acc_s ? acc_s + as : nullptr,
                      u_prim ? u_prim + us : nullptr, nullptr, tiny_h, h_anuga_sq, acc_p ? acc_p + as : nullptr, ext ? ext + as : nullptr,
                      acc_x ? acc_x + as : nullptr);
}

// blockIdx.y: the member.  mean[m][i] = acc[m][i] * s.v[m] for the n = 3 n_owned elements of a member.
__global__ void __launch_bounds__(ENS_OUT_BLOCK) ens_output_mean_kernel(int64_t n, const EnsPerMember s, const double *__restrict__ acc,
                                                                        double *__restrict__ mean) {
  const int64_t t = (int64_t)blockIdx.x * ENS_OUT_BLOCK + threadIdx.x;
  if (t >= n) return;
  const int64_t i = (int64_t)blockIdx.y * n + t;
  mean[i]         = acc[i] * s.v[blockIdx.y];
}

// blockIdx.y: the member.  One thread per site.
__global__ void __launch_bounds__(ENS_OUT_BLOCK) ens_series_observe_kernel(int S, int B, const int32_t *__restrict__ site_local, int64_t u_stride,
                                                                           const double *__restrict__ u, int64_t r, double *__restrict__ dlog) {
  const int s = blockIdx.x * ENS_OUT_BLOCK + threadIdx.x;
  if (s >= S) return;
  const int64_t m   = blockIdx.y;
  const double *um  = u + m * u_stride + 3 * (int64_t)site_local[s];
  const int64_t row = ((r * B + m) * S + s) * 3;
  const double  v0 = um[0], v1 = um[1], v2 = um[2];
  dlog[row + 0] = v0;
  dlog[row + 1] = v1;
  dlog[row + 2] = v2;
}

// One thread per owned cell, walking the B members; stats [popcount(comps)][3][n_owned] = (mean, min, max); inv_b = 1.0 / B, formed
// on the host.
__global__ void __launch_bounds__(ENS_OUT_BLOCK) ens_stats_kernel(int n_owned, const int32_t *__restrict__ o2l, int comps, int B, double inv_b,
                                                                  int64_t u_stride, const double *__restrict__ u, double *__restrict__ stats) {
  const int64_t o = (int64_t)blockIdx.x * ENS_OUT_BLOCK + threadIdx.x;
  if (o >= n_owned) return;
  // All three components are walked whatever `comps` asks for -- a row's components share its cache lines, and a loop body
  // without branches lets the loads of several members be in flight at once -- and only the planes asked for are stored.
  const double *x = u + 3 * (o2l ? (int64_t)o2l[o] : o);
  double        s[3], lo[3], hi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) s[c] = lo[c] = hi[c] = x[c];
#pragma unroll 4
  for (int m = 1; m < B; ++m) {
    x += u_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double xm = x[c];
      s[c]  = s[c] + xm;
      lo[c] = (xm < lo[c]) ? xm : lo[c];
      hi[c] = (xm > hi[c]) ? xm : hi[c];
    }
  }
  double *p = stats + o;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!(comps >> c & 1)) continue;
    p[0]                    = s[c] * inv_b;
    p[(int64_t)n_owned]     = lo[c];
    p[2 * (int64_t)n_owned] = hi[c];
    p += 3 * (int64_t)n_owned;
  }
}

}  // namespace rdyhip
