// The time-averaged output fields (rdyhip_output_mean_*: AccumulateOutputVar / ComputeMean of WriteXDMFOutput,
// src/xdmf_output.c:196-230), kept on the device: one accumulate launch per step for any subset of the three variables, one
// scaling launch per variable and output.
//
//   accumulate, for every owned cell o and its 3 components:
//     acc_s[o] = fma(dt, u_sol[loc(o)], acc_s[o])        the solution
//     acc_p[o] = fma(dt, pv(o),         acc_p[o])        the primitive variables (h, u, v)
//     acc_x[o] = fma(dt, ext[o],        acc_x[o])        the external sources
//   mean:  mean[i] = acc[i] * s,  s = 1 / accumulated time (formed on the host, as ComputeMean's VecScale)
//
// loc(o) = o where the owned cells are the first rows of the local vector, o2l[o] otherwise.  A null accumulator leaves its
// variable out.  pv(o) is the stored row pv_stored[o] while the evaluations store the primitive variables, and otherwise
// riemann_side(u_prev[loc(o)]) as primitive_variables_kernel (swe_kernels.h) forms it: the same bits a storing launch writes,
// without the 24 B/cell store in every RHS launch.  u_sol and u_prev are in general different arrays (after a fused Euler step:
// its output and its input); where they are the same pointer the row is read once.  The fmas are written out: the bits of
// axpy_owned_kernel's u += dt * f, which hipcc contracts to one v_fmac_f64 (rk_kernels.h says the same of its updates).
//
// Pure streams, 72 B per cell and variable (48 B for stored primitive variables plus their 24 B read).  (h, u, v) needs a whole
// row in one lane, so a lane takes a cell, not an element, in three 8-byte accesses per array.  Two cells per lane -- three
// 16-byte accesses per array, what rk_kernels.h found best for its element-wise streams -- was measured on an earlier build
// with both forms and was 2 to 5 % slower at every size (profiles/output_mean_ab_two_cells.txt; the cause was not measured --
// a conjecture: a lane's 48 bytes leave a wave's accesses at a 48-byte stride), so only this form exists.  The mean kernel is
// element-wise and keeps the 16-byte form.  Default cache policy throughout: the accumulators are read again by the next step's
// launch, the states by the next RHS; non-temporal accesses to the accumulators and the source were measured and are slower at
// every size (profiles/output_mean_ab_nontemporal.txt).  Figures of this kernel: profiles/output_mean_ab.txt, RESULTS_LOG
// section 18 -- 2.05 and 2.34 x axpy_owned_kernel at 0.36 M and 1 M cells, 3.17 x at 10 M, above its 3.0 x byte ratio.
// No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "swe_device.h"

namespace rdyhip {

constexpr int OUT_BLOCK = 256;

struct OutRow {
  double x, y, z;
};
__device__ __forceinline__ OutRow out_load(const double *__restrict__ p, int64_t row) {
  return OutRow{p[3 * row + 0], p[3 * row + 1], p[3 * row + 2]};
}
__device__ __forceinline__ void out_fma_store(double *__restrict__ acc, int64_t row, double dt, const OutRow &v) {
  acc[3 * row + 0] = fma(dt, v.x, acc[3 * row + 0]);
  acc[3 * row + 1] = fma(dt, v.y, acc[3 * row + 1]);
  acc[3 * row + 2] = fma(dt, v.z, acc[3 * row + 2]);
}
// one cell: owned row o, local row c
__device__ __forceinline__ void out_accumulate_cell(int64_t o, int64_t c, double dt, const double *__restrict__ u_sol, double *__restrict__ acc_s,
                                                    const double *__restrict__ u_prev, const double *__restrict__ pv_stored, double tiny_h,
                                                    double h_anuga_sq, double *__restrict__ acc_p, const double *__restrict__ ext,
                                                    double *__restrict__ acc_x) {
  const bool derive = acc_p && !pv_stored;
  OutRow     up{0.0, 0.0, 0.0};
  if (derive) up = out_load(u_prev, c);
  if (acc_s) {
    const OutRow us = (derive && u_sol == u_prev) ? up : out_load(u_sol, c);
    out_fma_store(acc_s, o, dt, us);
  }
  if (acc_p) {
    OutRow pv;
    if (derive) {
      const RiemannSide s = riemann_side(up.x, up.y, up.z, tiny_h, h_anuga_sq);
      pv                  = OutRow{s.h, s.u, s.v};
    } else {
      pv = out_load(pv_stored, o);
    }
    out_fma_store(acc_p, o, dt, pv);
  }
  if (acc_x) out_fma_store(acc_x, o, dt, out_load(ext, o));
}

// One thread per owned cell.
__global__ void output_accumulate_kernel(int n_owned, const int32_t *__restrict__ o2l, double dt, const double *__restrict__ u_sol,
                                         double *__restrict__ acc_s, const double *__restrict__ u_prev, const double *__restrict__ pv_stored,
                                         double tiny_h, double h_anuga_sq, double *__restrict__ acc_p, const double *__restrict__ ext,
                                         double *__restrict__ acc_x) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_owned) return;
  out_accumulate_cell(o, o2l ? (int64_t)o2l[o] : o, dt, u_sol, acc_s, u_prev, pv_stored, tiny_h, h_anuga_sq, acc_p, ext, acc_x);
}

// mean[i] = acc[i] * s for the n = 3 * n_owned elements; one thread per pair of elements when WIDE, with a scalar tail
template <bool WIDE>
__global__ void output_mean_kernel(int64_t n, double s, const double *__restrict__ acc, double *__restrict__ mean) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (WIDE) {
    const int64_t e = 2 * t;
    if (e + 1 < n) {
      const double2 a = *reinterpret_cast<const double2 *>(acc + e);
      double2       r;
      r.x = a.x * s;
      r.y = a.y * s;
      *reinterpret_cast<double2 *>(mean + e) = r;
    } else if (e < n) {
      mean[e] = acc[e] * s;
    }
  } else {
    if (t >= n) return;
    mean[t] = acc[t] * s;
  }
}

}  // namespace rdyhip
