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

// ---- the two kernel families: tracer_rhs_kernel (plain) and tracer_hr_kernel (hydrostatic reconstruction) ---------------------------
// Both read: shared prologue (cell_of_phase, swe_kernels.h; tracer_own_cell below), the family's own interior slot, the shared
// boundary slot (tracer_boundary_flux.h), the shared epilogue (tracer_epilogue.h), block_courant_reduce.  The prologue is two
// functions: with them every result keeps its bits.  The boundary slot and the epilogue are files included in place: as
// functions they change bits of F (see the two files).  "The edge counts" (acc += fl coef, the Courant candidate) stays where it
// is, once in the plain kernel and twice in the HR one: as a function it changes the NaN payloads that bflux holds for edges dry
// on both sides.  (What each form was measured to do: profiles/RESULTS_LOG.md section 32.)
//
// Phases (KernelArgs::phase, a run-time scalar: no further instantiations): every launch has one thread per owned cell, and a
// thread whose cell is not of the launch's phase (cell_of_phase) loads nothing but its neighbour ids, stores nothing and enters
// the reduction with best = 0.  A workgroup therefore has the same Courant bucket in every phase, and a launch with
// reset_diag == 0 merges into it (block_courant_reduce).

// The thread's own cell: its row of the state and, under the plain tracer path's rules (h < tiny_h => 0, no regularisation),
// its Riemann side and concentrations -- what the boundary slots and the source of BOTH families use.  Returns the local id.
// (Plain arrays, no struct: carried in one, two instantiations of tracer_hr_kernel take 6 VGPRs more and lose a wave per SIMD.)
template <int NT>
__device__ __forceinline__ int64_t tracer_own_cell(const KernelArgs &a, const double *__restrict__ u, int o, double *own, RiemannSide &self, double *self_c) {
  const int64_t c = a.o2l ? a.o2l[o] : o;
#pragma unroll
  for (int k = 0; k < 3 + NT; ++k) own[k] = u[(3 + NT) * c + k];
  self = riemann_side(own[0], own[1], own[2], a.tiny_h, 0.0);
  tracer_concentrations<NT>(own[0], own + 3, a.tiny_h, self_c);
  return c;
}

// ---- the plain family (rdyhip_tracers_enable) ------------------------------------------------------------------------------------
// One thread = one owned cell: the prologue prepares the cell's own row once, its up to S slots are walked in slot order -- the
// interior slot below is this family's own --, the source epilogue of ApplyTracerSourceSemiImplicit and the stores follow; the
// Courant bucket goes through block_courant_reduce with the `pos` table, so ties resolve as in swe_rhs_kernel.  f = F(u) only.
template <int S, int NT, bool UPWIND>
__global__ __launch_bounds__(BLOCK) void tracer_rhs_kernel(const KernelArgs a, const TracerArgs t, const double dt, const double *__restrict__ u) {
  constexpr bool HR = false;
  constexpr int  N  = 3 + NT;
  const int     i = xcd_block(a.xcd_chunks) * BLOCK + threadIdx.x;

  double best      = 0.0;
  int    best_slot = -1;
  int    o         = 0;

  bool           active = i < a.n_work;
  int32_t        id[S];
  const int32_t *nbr = RDY_COLD(a, nbr);
  if (active) {
    o      = i;
    active = cell_of_phase<S>(a, nbr, o, id);
  }
  if (active) {
    const int32_t *btype = RDY_COLD(a, btype);
    const double  *cn_ = RDY_COLD(a, cn), *sn_ = RDY_COLD(a, sn);
    double         own[N], self_c[NT];
    RiemannSide    self;
    const int64_t  c = tracer_own_cell<NT>(a, u, o, own, self, self_c);

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
#include "tracer_boundary_flux.h"
        wet = !(self.h < a.tiny_h && R.h < a.tiny_h);
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
#include "tracer_epilogue.h"
  }
  block_courant_reduce<BLOCK>(a, best, RDY_COLD(a, pos), (best_slot < 0 ? 0 : best_slot) * a.stride + o);
}

// ---- tracers under hydrostatic reconstruction (rdyhip_tracer_hr_enable) ---------------------------------------------------------
// ApplyTracerInteriorFluxHR + ApplyTracerSourceHRSemiImplicit (tracer_petsc.c:807-986, 1067-1154): the prologue, the boundary
// slot and the epilogue are tracer_rhs_kernel's own (the same functions, the same included files).  What this kernel states
// itself is three lines for the own cell (z_self, self_hr, self_wet_hr) and the interior slot; the epilogue drops the bed slope
// under `HR`:
//   velocities     of both cells in the ANUGA form hu h / (h^2 + h_anuga^2) under the HR operator's wet test h > tiny_h
//                  (869-875): riemann_side(..., h_anuga_sq) and hr_velocity_rule;  c_j = (h > tiny_h) ? h c_j / h : 0 (889-890)
//   depths         both reconstructed against max(zc_L, zc_R) (hr_reconstruct, swe_kernels.h); velocities and concentrations
//                  pass through, so the tracer components of tracer_roe_flux see h_rec c (892-893)
//   guards         the edge counts unless both ORIGINAL depths are below tiny_h (922); inside that, the N flux components and
//                  the Courant candidate only where a reconstructed depth exceeds tiny_h (939) -- with both at 0 the Roe
//                  solver returns 0 / 0, which a branch discards --; the own side's pressure correction
//                  0.5 g (h^2 - h_rec^2) (cn, sn) whenever the outer guard holds (964-977), after the edge's flux
//   boundary slots tracer_boundary_flux.h (operator_fluxes_petsc.c:79-93: HR is a no-op there), with the plain path's rule for
//                  the own cell (h < tiny_h => 0, no regularisation); the source keeps that rule too and has no bed slope
// The own cell therefore carries two rule sets; they differ only at h == tiny_h exactly and where h_anuga != 0.
template <int S, int NT, bool UPWIND>
__global__ __launch_bounds__(BLOCK) void tracer_hr_kernel(const KernelArgs a, const TracerArgs t, const double dt, const double *__restrict__ u) {
  constexpr bool HR = true;
  constexpr int  N  = 3 + NT;
  const int     i = xcd_block(a.xcd_chunks) * BLOCK + threadIdx.x;

  double best      = 0.0;
  int    best_slot = -1;
  int    o         = 0;

  bool           active = i < a.n_work;
  int32_t        id[S];
  const int32_t *nbr = RDY_COLD(a, nbr);
  if (active) {
    o      = i;
    active = cell_of_phase<S>(a, nbr, o, id);
  }
  if (active) {
    const int32_t *btype = RDY_COLD(a, btype);
    const double  *cn_ = RDY_COLD(a, cn), *sn_ = RDY_COLD(a, sn);
    double         own[N], self_c[NT];
    RiemannSide    self;
    const int64_t  c = tracer_own_cell<NT>(a, u, o, own, self, self_c);
    // interior edges: the HR operator's own cell (its concentrations are self_c under the strict test, selected where they are used)
    const double z_self  = a.zc_local[c];
    RiemannSide  self_hr = riemann_side(own[0], own[1], own[2], a.tiny_h, a.h_anuga_sq);
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
#include "tracer_boundary_flux.h"
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
#include "tracer_epilogue.h"
  }
  block_courant_reduce<BLOCK>(a, best, RDY_COLD(a, pos), (best_slot < 0 ? 0 : best_slot) * a.stride + o);
}

}  // namespace rdyhip
