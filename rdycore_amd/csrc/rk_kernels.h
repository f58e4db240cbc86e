// The vector updates of one classical Runge-Kutta step (rdyhip_rk4_step: TSStep_RK with the TSRK4 tableau,
// src/rdysetup.c:1187-1189) around the four RHS launches: one stage kernel per stage state, one combine kernel per step.
//
//   stage:   y[loc(o)] = fma(c, k[o], u0[loc(o)])                                            72 B per cell
//   combine: u[loc(o)] = fma(c4, k4[o], fma(c3, k3[o], fma(c2, k2[o], fma(c1, k1[o], u[loc(o)]))))   144 B per cell
//
// for every owned cell o and its 3 components; loc(o) = o where the owned cells are the first rows of the local vector,
// o2l[o] otherwise.  The fmas are written out, in the order in which a chain of axpy_owned_kernel launches applies them
// (hipcc contracts that kernel's u += dt * f to one v_fmac_f64): the same bits as copy + axpy per stage and four axpys at
// the end, in 360 B per cell and step instead of 648.
//
// Pure streams.  With the owned rows first, a lane moves 16 bytes per access (double2) while every pointer involved is
// 16-byte aligned (the launch checks), with a scalar tail: 3 * n_owned can be odd.  The 8-byte form is the same arithmetic
// element by element.  Loads and stores take the default cache policy -- y is read by the RHS launch that follows, u by the
// next step's, the stage kernel's k has just been written -- except the 16-byte loads of k1..k4 in the combine kernel, their
// last reader: with the non-temporal hint that kernel takes 1.82 x the time of axpy_owned_kernel at 10 M cells, 2.10 x
// without; where the stage vectors fit on chip the hint costs a little (1.64 x against 1.60 x at 1 M cells)
// (profiles/RESULTS_LOG.md section 17).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rdyhip {

constexpr int RK_BLOCK = 256;

typedef double rk_double2 __attribute__((ext_vector_type(2)));
// 16 bytes that nobody reads again
__device__ inline double2 rk_load2_once(const double *p) {
  const rk_double2 v = __builtin_nontemporal_load(reinterpret_cast<const rk_double2 *>(p));
  double2          r;
  r.x = v.x;
  r.y = v.y;
  return r;
}

// Owned rows first (o2l == nullptr): the launch covers all n_all = 3 * num_cells elements of y -- the first n_own =
// 3 * n_owned get the update, the rest (the ghost rows) are copied from u0 -- or only the owned ones (n_all == n_own) where
// an exchange fills every ghost row anyway.  One thread per pair of elements when WIDE, per element otherwise.
// With o2l: one thread per owned element; the ghost rows are the caller's (a device-to-device copy in front).
template <bool WIDE>
__global__ void rk4_stage_kernel(int64_t n_own, int64_t n_all, const int32_t *__restrict__ o2l, double c, const double *__restrict__ k,
                                 const double *__restrict__ u0, double *__restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o2l) {
    if (t >= n_own) return;
    const int64_t o = t / 3;
    const int64_t j = 3 * (int64_t)o2l[o] + (t - 3 * o);
    y[j]            = fma(c, k[t], u0[j]);
    return;
  }
  if constexpr (WIDE) {
    const int64_t e = 2 * t;
    if (e + 1 < n_own) {
      const double2 kk = *reinterpret_cast<const double2 *>(k + e);
      const double2 uu = *reinterpret_cast<const double2 *>(u0 + e);
      double2       r;
      r.x = fma(c, kk.x, uu.x);
      r.y = fma(c, kk.y, uu.y);
      *reinterpret_cast<double2 *>(y + e) = r;
    } else if (e >= n_own && e + 1 < n_all) {
      *reinterpret_cast<double2 *>(y + e) = *reinterpret_cast<const double2 *>(u0 + e);
    } else {
      // the pair that straddles the end of the owned rows, and the last element of an odd count
      for (int64_t i = e; i < e + 2 && i < n_all; ++i) y[i] = i < n_own ? fma(c, k[i], u0[i]) : u0[i];
    }
  } else {
    if (t >= n_all) return;
    y[t] = t < n_own ? fma(c, k[t], u0[t]) : u0[t];
  }
}

template <bool WIDE>
__global__ void rk4_combine_kernel(int64_t n_own, const int32_t *__restrict__ o2l, double c1, double c2, double c3, double c4,
                                   const double *__restrict__ k1, const double *__restrict__ k2, const double *__restrict__ k3,
                                   const double *__restrict__ k4, double *__restrict__ u) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o2l) {
    if (t >= n_own) return;
    const int64_t o = t / 3;
    const int64_t j = 3 * (int64_t)o2l[o] + (t - 3 * o);
    u[j]            = fma(c4, k4[t], fma(c3, k3[t], fma(c2, k2[t], fma(c1, k1[t], u[j]))));
    return;
  }
  if constexpr (WIDE) {
    const int64_t e = 2 * t;
    if (e + 1 < n_own) {
      const double2 a = rk_load2_once(k1 + e), b = rk_load2_once(k2 + e), g = rk_load2_once(k3 + e), d = rk_load2_once(k4 + e);
      double2       r = *reinterpret_cast<const double2 *>(u + e);
      r.x = fma(c4, d.x, fma(c3, g.x, fma(c2, b.x, fma(c1, a.x, r.x))));
      r.y = fma(c4, d.y, fma(c3, g.y, fma(c2, b.y, fma(c1, a.y, r.y))));
      *reinterpret_cast<double2 *>(u + e) = r;
    } else if (e < n_own) {
      u[e] = fma(c4, k4[e], fma(c3, k3[e], fma(c2, k2[e], fma(c1, k1[e], u[e]))));
    }
  } else {
    if (t >= n_own) return;
    u[t] = fma(c4, k4[t], fma(c3, k3[t], fma(c2, k2[t], fma(c1, k1[t], u[t]))));
  }
}

}  // namespace rdyhip
