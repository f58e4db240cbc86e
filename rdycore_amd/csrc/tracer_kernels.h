// Shallow water with advected tracers (sediment classes, salinity, temperature) for gfx950: the first-order right-hand side
// of the reference's PETSc tracer path (src/tracer/tracer_petsc.c, src/tracer/tracer_roe_flux_petsc.h) in one kernel of the
// cell-centric form (swe_rhs_kernel, swe_kernels.h): one thread = one owned cell, every edge of the cell evaluated by that
// thread in slot order (= the reference's loop order), so the per-cell sum has a fixed order and needs no atomics.
//
// The state is [cell][3 + NT] = (h, hu, hv, h c_0 ...): the reference's one Vec with block size n_dof.  NT is a template
// argument: the rows, the accumulators and the concentrations are per-thread arrays with compile-time indices and live in
// registers (a run-time tracer count would put them in scratch).  A row's 3 + NT doubles are loaded and stored back to back.
//
// The flow part reuses the operator's own tables through KernelArgs / ColdArgs (slot tables, Manning n, the [owned][3]
// external source, the Courant buckets); what only this path has travels in TracerArgs.  The inline functions of
// swe_device.h and swe_kernels.h are called as they are; the flow part of the flux is roe_flux_with() (swe_device.h), whose
// hook hands the tracer components the eigenvalue and wave terms they need (roe_flux() itself is the same body with an
// empty hook, so the SWE kernels' machine code is what it was).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdyhip.h"
#include "swe_device.h"
#include "swe_kernels.h"

namespace rdyhip {

// what the tracer kernel reads and writes beyond KernelArgs (N = 3 + NT values per row)
struct TracerArgs {
  const double *bvalues;  // [K][N] Dirichlet values (h, hu, hv, h c_0 ...) of boundary edge k
  double       *bflux;    // [K][N] flux through boundary edge k (edges whose left cell is owned)
  const double *src;      // [n_owned][NT] tracer sources
  double       *pv;       // [n_owned][N] (h, u, v, c_0 ...) or nullptr: nobody has asked for them
  double       *f;        // [n_owned][N] or nullptr (an Euler step whose caller wants no F)
  double       *u_out;    // [num_cells][N] or nullptr: owned rows = fma(dt, F, u)
};

// DENSITY_OF_WATER and the erosion / deposition constants of ApplyTracerSourceSemiImplicit (tracer_petsc.c:633-637)
constexpr double TRACER_RHO_WATER       = 1000.0;
constexpr double TRACER_KP              = 0.001;
constexpr double TRACER_SETTLING        = 0.01;
constexpr double TRACER_TAU_EROSION     = 0.1;
constexpr double TRACER_TAU_DEPOSITION  = 1000.0;

// ComputeRiemannVelocitiesAndConcentration (tracer_petsc.c:105-128) for the concentrations of one state: zero below
// tiny_h, else h c_i / h with the reciprocal taken once.  (The velocities are riemann_side(..., h_anuga_sq = 0).)
template <int NT>
__device__ __forceinline__ void tracer_concentrations(double h, const double *hc, double tiny_h, double *c) {
  const double inv = rdy_rcp(h);
#pragma unroll
  for (int j = 0; j < NT; ++j) c[j] = (h < tiny_h) ? 0.0 : hc[j] * inv;
}

// ComputeTracerRoeFlux / ComputeUpwindTracerRoeFlux (tracer_roe_flux_petsc.h:17-119, 129-206) for one edge.  The flow
// components are ComputeSWERoeFlux as roe_flux_with() (swe_device.h) evaluates it; in its hook tracer j adds
//   Roe:     cihat = (sqrt(hl) cl + sqrt(hr) cr) / (sqrt(hl) + sqrt(hr)),  dW_j = (cr hr - cl hl) - cihat (hr - hl),
//            flux_j = 0.5 (hl uperp_l cl + hr uperp_r cr) - 0.5 (cihat A0 dW0 + cihat A2 dW2 + A1 dW_j)
//   upwind:  flux_j = F_h (F_h >= 0 ? cl : cr), F_h the Roe mass flux
// fl[0..2] flow, fl[3..] tracers; returns amax.
template <int NT, bool UPWIND>
__device__ __forceinline__ double tracer_roe_flux(const RiemannSide &L, const RiemannSide &R, const double *cl_, const double *cr_, double sn, double cn,
                                                  double *fl) {
  const RoeFlux f = roe_flux_with(L, R, sn, cn, [&](const RoeWaves &w, const RoeFlux &o) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (UPWIND) {
        fl[3 + j] = o.f0 * (o.f0 >= 0.0 ? cl_[j] : cr_[j]);
      } else {
        const double cihat = sum_of_products(w.duml, cl_[j], w.dumr, cr_[j]) * w.inv_sum;
        const double dwj   = (cr_[j] * R.h - cl_[j] * L.h) - cihat * w.dh;
        fl[3 + j]          = 0.5 * (w.ql * cl_[j] + w.qr * cr_[j] - cihat * w.w0 - cihat * w.w2 - w.a2 * dwj);
      }
    }
  });
  fl[0] = f.f0, fl[1] = f.f1, fl[2] = f.f2;
  return f.amax;
}

// One thread = one owned cell: the cell's own row is prepared once, its up to S slots are walked in slot order, the source
// epilogue of ApplyTracerSourceSemiImplicit (tracer_petsc.c:617-737) and the stores follow; the Courant bucket goes through
// block_courant_reduce with the `pos` table, so ties resolve as in swe_rhs_kernel.  f = F(u) only.
// Phases (KernelArgs::phase, a run-time scalar: no further instantiations): every launch has one thread per owned cell, and a
// thread whose cell is not of the launch's phase -- ghost adjacency is the NBR_GHOST bit of its neighbour ids, as in
// swe_rhs_kernel -- loads and stores nothing and enters the reduction with best = 0.  A workgroup therefore has the same
// Courant bucket in every phase, and a launch with reset_diag == 0 merges into it (block_courant_reduce).
template <int S, int NT, bool UPWIND>
__global__ __launch_bounds__(BLOCK) void tracer_rhs_kernel(const KernelArgs a, const TracerArgs t, const double dt, const double *__restrict__ u) {
  constexpr int N = 3 + NT;
  const int     i = xcd_block(a.xcd_chunks) * BLOCK + threadIdx.x;

  double best      = 0.0;
  int    best_slot = -1;
  int    o         = 0;

  bool           active = i < a.n_work;
  int32_t        id[S];
  const int32_t *nbr = RDY_COLD(a, nbr);
  if (active) {
    o              = i;
    bool has_ghost = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      id[s] = nbr[s * a.stride + o];
      has_ghost |= (id[s] >= 0) && (id[s] & NBR_GHOST);
    }
    // a cell of the other phase: nothing but its neighbour ids is loaded, nothing is stored (a.phase is uniform per launch)
    if (a.phase == RDYHIP_PHASE_INTERIOR && has_ghost) active = false;
    if (a.phase == RDYHIP_PHASE_HALO && !has_ghost) active = false;
  }
  if (active) {
    const int32_t *btype = RDY_COLD(a, btype);
    const double  *cn_ = RDY_COLD(a, cn), *sn_ = RDY_COLD(a, sn);

    const int64_t c = a.o2l ? a.o2l[o] : o;
    double        own[N];
#pragma unroll
    for (int k = 0; k < N; ++k) own[k] = u[N * c + k];
    const RiemannSide self = riemann_side(own[0], own[1], own[2], a.tiny_h, 0.0);
    double            self_c[NT];
    tracer_concentrations<NT>(own[0], own + 3, a.tiny_h, self_c);

    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;

#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int32_t nid = id[s];
      if (nid == NBR_EMPTY) continue;  // a triangle in the 4-slot layout, or an outer edge that belongs to no boundary
      const double cn   = cn_[s * a.stride + o];
      const double sn   = sn_[s * a.stride + o];
      const double coef = a.coef[s * a.stride + o];
      const double cfac = fabs(coef);  // len / area_self: the max over an edge's two cells is len / min(area_l, area_r)
      double       fl[N], amax;
      bool         wet;
      if (nid >= 0) {
        const int64_t n = nid & NBR_MASK;
        double        oth[N];
#pragma unroll
        for (int k = 0; k < N; ++k) oth[k] = u[N * n + k];
        const RiemannSide other = riemann_side(oth[0], oth[1], oth[2], a.tiny_h, 0.0);
        double            other_c[NT];
        tracer_concentrations<NT>(oth[0], oth + 3, a.tiny_h, other_c);
        const bool  self_left = coef < 0.0;
        RiemannSide L, R;
        orient_sides(self, other, self_left, L, R);
        double cl[NT], cr[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          cl[j] = self_left ? self_c[j] : other_c[j];
          cr[j] = self_left ? other_c[j] : self_c[j];
        }
        amax = tracer_roe_flux<NT, UPWIND>(L, R, cl, cr, sn, cn, fl);
        wet  = !(R.h < a.tiny_h && L.h < a.tiny_h);
      } else {
        // ApplyTracerBoundaryFlux (tracer_petsc.c:405-525): the cell is the left one.  Critical outflow is refused at
        // rdyhip_tracers_enable (472-474), so a type that is not Dirichlet is reflecting.
        const int64_t k = -1 - nid;
        RiemannSide   R;
        double        cr[NT];
        if (btype[k] == RDYHIP_CONDITION_DIRICHLET) {
          double bv[N];
#pragma unroll
          for (int q = 0; q < N; ++q) bv[q] = t.bvalues[N * k + q];
          R = riemann_side(bv[0], bv[1], bv[2], a.tiny_h, 0.0);
          tracer_concentrations<NT>(bv[0], bv + 3, a.tiny_h, cr);
        } else {  // ApplyTracerReflectingBC (362-395): h and c_i copied, the velocity mirrored
          const double dum1 = sn * sn - cn * cn;
          const double dum2 = 2.0 * sn * cn;
          R.h               = self.h;
          R.u               = self.u * dum1 - self.v * dum2;
          R.v               = -self.u * dum2 - self.v * dum1;
          R.sqh             = self.sqh;
          R.c               = self.c;
#pragma unroll
          for (int j = 0; j < NT; ++j) cr[j] = self_c[j];
        }
        amax = tracer_roe_flux<NT, UPWIND>(self, R, self_c, cr, sn, cn, fl);
        wet  = !(self.h < a.tiny_h && R.h < a.tiny_h);
#pragma unroll
        for (int q = 0; q < N; ++q) t.bflux[N * k + q] = fl[q];
      }
      if (wet) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += fl[k] * coef;
        const double cnum = amax * cfac * dt;
        if (cnum > best) {
          best      = cnum;
          best_slot = s;
        }
      }
    }

    // sources: bed slope, semi-implicit friction on the pre-source momentum sums, erosion - deposition for wet cells
    const double h = own[0];
    const double n = a.mannings[o];
    double       bedx, bedy, tbx, tby;
    cell_source<RDYHIP_SOURCE_SEMI_IMPLICIT>(a, dt, h, own[1], own[2], acc[1], acc[2], a.dzdx[o], a.dzdy[o], n, bedx, bedy, tbx, tby);
    double F[N];
    F[0] = acc[0] + a.extsrc[3 * (int64_t)o + 0];
    F[1] = acc[1] + (-bedx - tbx + a.extsrc[3 * (int64_t)o + 1]);
    F[2] = acc[2] + (-bedy - tby + a.extsrc[3 * (int64_t)o + 2]);
    const bool   cell_wet = h >= a.tiny_h;
    const double Cd       = GRAVITY * (n * n) * rcbrt(h);
    const double tau_b    = 0.5 * TRACER_RHO_WATER * Cd * (self.u * self.u + self.v * self.v);  // h >= tiny_h: self.u = hu / h
    const double ei       = TRACER_KP * (tau_b - TRACER_TAU_EROSION) / TRACER_TAU_EROSION;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double di = TRACER_SETTLING * self_c[j] * (1.0 - tau_b / TRACER_TAU_DEPOSITION);
      F[3 + j]        = cell_wet ? acc[3 + j] + ((ei - di) + t.src[NT * (int64_t)o + j]) : acc[3 + j];
    }

    if (t.f) {
#pragma unroll
      for (int k = 0; k < N; ++k) RDY_ST(&t.f[N * (int64_t)o + k], F[k]);
    }
    // primitive variables (tracer_petsc.c:715-724): the regularised velocities, c_i = h c_i / h, all zero below tiny_h
    if (t.pv) {
      const RiemannSide p = riemann_side(h, own[1], own[2], a.tiny_h, a.h_anuga_sq);
      RDY_ST(&t.pv[N * (int64_t)o + 0], h);
      RDY_ST(&t.pv[N * (int64_t)o + 1], p.u);
      RDY_ST(&t.pv[N * (int64_t)o + 2], p.v);
#pragma unroll
      for (int j = 0; j < NT; ++j) RDY_ST(&t.pv[N * (int64_t)o + 3 + j], self_c[j]);
    }
    if (t.u_out) {
#pragma unroll
      for (int k = 0; k < N; ++k) RDY_ST(&t.u_out[N * c + k], fma(dt, F[k], own[k]));
    }
  }
  block_courant_reduce<BLOCK>(a, best, RDY_COLD(a, pos), (best_slot < 0 ? 0 : best_slot) * a.stride + o);
}

// ---- tracers under hydrostatic reconstruction (rdyhip_tracer_hr_enable) ---------------------------------------------------------
// ApplyTracerInteriorFluxHR + ApplyTracerSourceHRSemiImplicit (tracer_petsc.c:807-986, 1067-1154) in the shape of
// tracer_rhs_kernel: the same thread per owned cell, slot order, phases, TracerArgs, stores and Courant bucket.  What differs
// is the interior slot and the bed slope:
//   velocities     of both cells in the ANUGA form hu h / (h^2 + h_anuga^2) under the HR operator's wet test h > tiny_h
//                  (869-875): riemann_side(..., h_anuga_sq) and hr_velocity_rule;  c_j = (h > tiny_h) ? h c_j / h : 0 (889-890)
//   depths         both reconstructed against max(zc_L, zc_R) (hr_reconstruct, swe_kernels.h); velocities and concentrations
//                  pass through, so the tracer components of tracer_roe_flux see h_rec c (892-893)
//   guards         the edge counts unless both ORIGINAL depths are below tiny_h (922); inside that, the N flux components and
//                  the Courant candidate only where a reconstructed depth exceeds tiny_h (939) -- with both at 0 the Roe
//                  solver returns 0 / 0, which a branch discards --; the own side's pressure correction
//                  0.5 g (h^2 - h_rec^2) (cn, sn) whenever the outer guard holds (964-977), after the edge's flux
//   boundary slots as in tracer_rhs_kernel (operator_fluxes_petsc.c:79-93: HR is a no-op there) with that kernel's rule for
//                  the own cell (h < tiny_h => 0, no regularisation); the source keeps that rule too and has no bed slope
// The own cell therefore carries two rule sets; they differ only at h == tiny_h exactly and where h_anuga != 0.
template <int S, int NT, bool UPWIND>
__global__ __launch_bounds__(BLOCK) void tracer_hr_kernel(const KernelArgs a, const TracerArgs t, const double dt, const double *__restrict__ u) {
  constexpr int N = 3 + NT;
  const int     i = xcd_block(a.xcd_chunks) * BLOCK + threadIdx.x;

  double best      = 0.0;
  int    best_slot = -1;
  int    o         = 0;

  bool           active = i < a.n_work;
  int32_t        id[S];
  const int32_t *nbr = RDY_COLD(a, nbr);
  if (active) {
    o              = i;
    bool has_ghost = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      id[s] = nbr[s * a.stride + o];
      has_ghost |= (id[s] >= 0) && (id[s] & NBR_GHOST);
    }
    if (a.phase == RDYHIP_PHASE_INTERIOR && has_ghost) active = false;
    if (a.phase == RDYHIP_PHASE_HALO && !has_ghost) active = false;
  }
  if (active) {
    const int32_t *btype = RDY_COLD(a, btype);
    const double  *cn_ = RDY_COLD(a, cn), *sn_ = RDY_COLD(a, sn);

    const int64_t c = a.o2l ? a.o2l[o] : o;
    double        own[N];
#pragma unroll
    for (int k = 0; k < N; ++k) own[k] = u[N * c + k];
    const double z_self = a.zc_local[c];
    // boundary edges and the source: the plain tracer path's own cell
    const RiemannSide self = riemann_side(own[0], own[1], own[2], a.tiny_h, 0.0);
    double            self_c[NT];
    tracer_concentrations<NT>(own[0], own + 3, a.tiny_h, self_c);
    // interior edges: the HR operator's (its concentrations are self_c under the strict test, selected where they are used)
    RiemannSide self_hr = riemann_side(own[0], own[1], own[2], a.tiny_h, a.h_anuga_sq);
    hr_velocity_rule(self_hr, a.tiny_h);
    const bool self_wet_hr = own[0] > a.tiny_h;

    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;

#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int32_t nid = id[s];
      if (nid == NBR_EMPTY) continue;
      const double cn   = cn_[s * a.stride + o];
      const double sn   = sn_[s * a.stride + o];
      const double coef = a.coef[s * a.stride + o];
      const double cfac = fabs(coef);
      double       fl[N], amax;
      if (nid >= 0) {
        const int64_t n = nid & NBR_MASK;
        double        oth[N];
#pragma unroll
        for (int k = 0; k < N; ++k) oth[k] = u[N * n + k];
        const double z_other = a.zc_local[n];
        RiemannSide  other   = riemann_side(oth[0], oth[1], oth[2], a.tiny_h, a.h_anuga_sq);
        hr_velocity_rule(other, a.tiny_h);
        const bool   other_wet = oth[0] > a.tiny_h;
        const double inv       = rdy_rcp(oth[0]);
        const bool   self_left = coef < 0.0;
        RiemannSide  L, R, Lr, Rr;
        orient_sides(self_hr, other, self_left, L, R);
        double cl[NT], cr[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const double cs = self_wet_hr ? self_c[j] : 0.0;
          const double co = other_wet ? oth[3 + j] * inv : 0.0;
          cl[j]           = self_left ? cs : co;
          cr[j]           = self_left ? co : cs;
        }
        hr_reconstruct(L, R, self_left ? z_self : z_other, self_left ? z_other : z_self, Lr, Rr);
        amax = tracer_roe_flux<NT, UPWIND>(Lr, Rr, cl, cr, sn, cn, fl);
        if (!(R.h < a.tiny_h && L.h < a.tiny_h)) {
          if (Lr.h > a.tiny_h || Rr.h > a.tiny_h) {
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] += fl[k] * coef;
            const double cnum = amax * cfac * dt;
            if (cnum > best) {
              best      = cnum;
              best_slot = s;
            }
          }
          const double h_rec = self_left ? Lr.h : Rr.h;
          const double corr  = 0.5 * GRAVITY * (own[0] * own[0] - h_rec * h_rec);
          acc[1] += corr * cn * coef;
          acc[2] += corr * sn * coef;
        }
      } else {
        // ApplyTracerBoundaryFlux, exactly as in tracer_rhs_kernel
        const int64_t k = -1 - nid;
        RiemannSide   R;
        double        cr[NT];
        if (btype[k] == RDYHIP_CONDITION_DIRICHLET) {
          double bv[N];
#pragma unroll
          for (int q = 0; q < N; ++q) bv[q] = t.bvalues[N * k + q];
          R = riemann_side(bv[0], bv[1], bv[2], a.tiny_h, 0.0);
          tracer_concentrations<NT>(bv[0], bv + 3, a.tiny_h, cr);
        } else {
          const double dum1 = sn * sn - cn * cn;
          const double dum2 = 2.0 * sn * cn;
          R.h               = self.h;
          R.u               = self.u * dum1 - self.v * dum2;
          R.v               = -self.u * dum2 - self.v * dum1;
          R.sqh             = self.sqh;
          R.c               = self.c;
#pragma unroll
          for (int j = 0; j < NT; ++j) cr[j] = self_c[j];
        }
        amax = tracer_roe_flux<NT, UPWIND>(self, R, self_c, cr, sn, cn, fl);
#pragma unroll
        for (int q = 0; q < N; ++q) t.bflux[N * k + q] = fl[q];
        if (!(self.h < a.tiny_h && R.h < a.tiny_h)) {
#pragma unroll
          for (int k2 = 0; k2 < N; ++k2) acc[k2] += fl[k2] * coef;
          const double cnum = amax * cfac * dt;
          if (cnum > best) {
            best      = cnum;
            best_slot = s;
          }
        }
      }
    }

    // sources (ApplyTracerSourceHRSemiImplicit): no bed slope; friction, erosion and deposition as in tracer_rhs_kernel
    const double h = own[0];
    const double n = a.mannings[o];
    double       bedx, bedy, tbx, tby;
    cell_source<RDYHIP_SOURCE_SEMI_IMPLICIT>(a, dt, h, own[1], own[2], acc[1], acc[2], 0.0, 0.0, n, bedx, bedy, tbx, tby);
    double F[N];
    F[0] = acc[0] + a.extsrc[3 * (int64_t)o + 0];
    F[1] = acc[1] + (-bedx - tbx + a.extsrc[3 * (int64_t)o + 1]);
    F[2] = acc[2] + (-bedy - tby + a.extsrc[3 * (int64_t)o + 2]);
    const bool   cell_wet = h >= a.tiny_h;
    const double Cd       = GRAVITY * (n * n) * rcbrt(h);
    const double tau_b    = 0.5 * TRACER_RHO_WATER * Cd * (self.u * self.u + self.v * self.v);
    const double ei       = TRACER_KP * (tau_b - TRACER_TAU_EROSION) / TRACER_TAU_EROSION;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double di = TRACER_SETTLING * self_c[j] * (1.0 - tau_b / TRACER_TAU_DEPOSITION);
      F[3 + j]        = cell_wet ? acc[3 + j] + ((ei - di) + t.src[NT * (int64_t)o + j]) : acc[3 + j];
    }

    if (t.f) {
#pragma unroll
      for (int k = 0; k < N; ++k) RDY_ST(&t.f[N * (int64_t)o + k], F[k]);
    }
    if (t.pv) {
      const RiemannSide p = riemann_side(h, own[1], own[2], a.tiny_h, a.h_anuga_sq);
      RDY_ST(&t.pv[N * (int64_t)o + 0], h);
      RDY_ST(&t.pv[N * (int64_t)o + 1], p.u);
      RDY_ST(&t.pv[N * (int64_t)o + 2], p.v);
#pragma unroll
      for (int j = 0; j < NT; ++j) RDY_ST(&t.pv[N * (int64_t)o + 3 + j], self_c[j]);
    }
    if (t.u_out) {
#pragma unroll
      for (int k = 0; k < N; ++k) RDY_ST(&t.u_out[N * c + k], fma(dt, F[k], own[k]));
    }
  }
  block_courant_reduce<BLOCK>(a, best, RDY_COLD(a, pos), (best_slot < 0 ? 0 : best_slot) * a.stride + o);
}

}  // namespace rdyhip
