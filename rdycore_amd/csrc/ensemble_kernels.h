// Ensembles for gfx950: B simulations on ONE mesh (the reference's `ensemble:` section, src/ensemble.c:5-84, where each member
// gets a communicator, a mesh copy and an operator of its own) evaluated by ONE launch of a kernel of the cell-centric form
// (swe_rhs_kernel, swe_kernels.h): one thread = one owned cell, every edge of the cell evaluated by that thread in slot order
// (= the reference's loop order), so a member's per-cell sum has a fixed order and needs no atomics.
//
// What a cell reads is of two kinds.  Geometry -- neighbour ids, cn, sn, coef, the boundary edges' condition types, bed slopes,
// the local id: about 100 B -- is the same for every member; the thread loads it ONCE and keeps it in registers.  Member data --
// its own row and its neighbours' rows of the member's state, Manning's n, the source row, F / u_out: about 80 B -- is walked
// member by member with that geometry.  A launch of B members so moves about 80 + 100 / B bytes per cell-update where B
// launches of the cell kernel move about 180.
//
// State: u [B][num_cells][3], F [B][n_owned][3], member-major: member m's slice is an ordinary SWE state.  The grid is
// (blocks of BLOCK cells, G): workgroup (x, g) walks members g P .. min(B, (g + 1) P) - 1 of its block's cells, P members per
// group (rdyhip_ensemble_enable chooses G: few cells -> many groups, so that a small mesh still fills the CUs; many cells ->
// up to ENSEMBLE_MAX_PER_GROUP members per thread, so that the geometry loads are shared).
//
// Courant diagnostic: one bucket per (member, wave), overwritten by every evaluation.  A wave reduces its 64 cells with
// shuffles alone: block_courant_reduce would cost two workgroup barriers per member.  Ties go to the edge that comes first in
// the reference's loop (the `pos` table, as in swe_rhs_kernel); ensemble_courant_finalize_kernel merges a member's buckets.
//
// The inline functions of swe_device.h and swe_kernels.h are called as they are; KernelArgs / ColdArgs carry the operator's
// shared tables, what only this path has travels in EnsembleArgs.
//
// Two kernel families share all of the above: ensemble_rhs_kernel (rdyhip_ensemble_enable) and, for operators created with
// hydrostatic reconstruction, ensemble_hr_kernel (rdyhip_ens_hr_enable), whose geometry holds bed elevations where the bed
// slopes were.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdyhip.h"
#include "swe_device.h"
#include "swe_kernels.h"

namespace rdyhip {

// The group rule of rdyhip_ensemble_enable (measured: profiles/RESULTS_LOG.md section 23).  Workgroups from which a launch stops
// splitting the members into more groups: 4 per CU on 256 CUs
constexpr int ENSEMBLE_MIN_WORKGROUPS = 1024;
// Members a thread walks at most: the geometry's share of a cell-update's bytes falls as 100 / P while a workgroup's run time,
// and with it the tail of the launch's last round, grows as P
constexpr int ENSEMBLE_MAX_PER_GROUP  = 8;
constexpr int ENSEMBLE_WAVES          = BLOCK / 64;  // Courant buckets per workgroup and member

// what the ensemble kernel reads and writes beyond KernelArgs (B members, K boundary edges)
struct EnsembleArgs {
  const double *mannings;  // [B][n_owned]
  const double *extsrc;    // [B][n_owned][3]
  const double *bvalues;   // [B][K][3]
  double       *bflux;     // [B][K][3] flux through boundary edge k (edges whose left cell is owned)
  double       *blk_max;   // [B][n_buckets] the Courant diagnostic: (max, first position) of every wave
  int32_t      *blk_pos;   // [B][n_buckets]
  double       *f;         // [B][n_owned][3], or nullptr (an Euler step whose caller wants no F)
  double       *u_out;     // EULER: [B][num_cells][3], owned rows = fma(dt_m, F, u)
  int64_t       u_stride;  // 3 num_cells: doubles between two members' states
  int64_t       k_stride;  // 3 K
  int32_t       n_members, per_group, n_buckets;
  double        dts[RDYHIP_MAX_ENSEMBLE_MEMBERS];  // one dt per member, by value
};

template <int S, int SRC, bool EULER>
__global__ __launch_bounds__(BLOCK) void ensemble_rhs_kernel(const KernelArgs a, const EnsembleArgs t, const double *__restrict__ u) {
  const int  i      = xcd_block(a.xcd_chunks) * BLOCK + threadIdx.x;
  const bool active = i < a.n_work;
  const int  o      = active ? i : 0;
  const int  lane   = threadIdx.x & 63;

  // ---- the cell's geometry, once for all members of the group
  int32_t id[S], bt[S];
  double  cn[S], sn[S], coef[S];
  double  dzdx = 0.0, dzdy = 0.0;
  int64_t c    = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    id[s] = NBR_EMPTY;
    bt[s] = 0;
    cn[s] = sn[s] = coef[s] = 0.0;
  }
  if (active) {
    const int32_t *nbr = RDY_COLD(a, nbr), *btype = RDY_COLD(a, btype);
    const double  *cn_ = RDY_COLD(a, cn), *sn_ = RDY_COLD(a, sn);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      id[s]   = nbr[s * a.stride + o];
      cn[s]   = cn_[s * a.stride + o];
      sn[s]   = sn_[s * a.stride + o];
      coef[s] = RDY_LD(&a.coef[s * a.stride + o]);
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (id[s] < 0 && id[s] != NBR_EMPTY) bt[s] = btype[-1 - id[s]];
    dzdx = RDY_LD(&a.dzdx[o]);
    dzdy = RDY_LD(&a.dzdy[o]);
    c    = a.o2l ? a.o2l[o] : o;
  }
  const int32_t *pos    = RDY_COLD(a, pos);
  const int      m0     = blockIdx.y * t.per_group;
  const int      m1     = min(t.n_members, m0 + t.per_group);
  const int      bucket = blockIdx.x * ENSEMBLE_WAVES + (threadIdx.x >> 6);

#pragma unroll 1
  for (int m = m0; m < m1; ++m) {
    const double  dt = t.dts[m];
    const double *um = u + (int64_t)m * t.u_stride;
    double        best      = 0.0;  // largest Courant number of this cell's edges (> 0 only)
    int           best_slot = -1;
    if (active) {
      const double      h    = um[3 * c + 0];
      const double      hu   = um[3 * c + 1];
      const double      hv   = um[3 * c + 2];
      const RiemannSide self = riemann_side(h, hu, hv, a.tiny_h, a.h_anuga_sq);
      double            acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int32_t nid = id[s];
        if (nid == NBR_EMPTY) continue;  // a triangle in the 4-slot layout, or an outer edge that belongs to no boundary
        RoeFlux      fl;
        bool         wet;
        const double cfac = fabs(coef[s]);  // len / area_self: the max over an edge's two cells is len / min(area_l, area_r)
        if (nid >= 0) {
          const int64_t     n     = nid & NBR_MASK;
          const RiemannSide other = riemann_side(um[3 * n + 0], um[3 * n + 1], um[3 * n + 2], a.tiny_h, a.h_anuga_sq);
          const bool        self_left = coef[s] < 0.0;
          RiemannSide       L, R;
          orient_sides(self, other, self_left, L, R);
          fl  = roe_flux(L, R, sn[s], cn[s]);
          wet = !(R.h < a.tiny_h && L.h < a.tiny_h);
        } else {
          const int64_t      k  = (int64_t)m * t.k_stride + 3 * (int64_t)(-1 - nid);
          const BoundaryFlux bf = boundary_flux(bt[s], true, self, t.bvalues + k, sn[s], cn[s], a.tiny_h, a.h_anuga_sq);
          fl                    = bf.flux;
          wet                   = bf.wet;
          t.bflux[k + 0]        = fl.f0;  // boundary_fluxes[b], swe_petsc.c:574
          t.bflux[k + 1]        = fl.f1;
          t.bflux[k + 2]        = fl.f2;
        }
        if (wet) {
          acc0 += fl.f0 * coef[s];
          acc1 += fl.f1 * coef[s];
          acc2 += fl.f2 * coef[s];
          const double cnum = fl.amax * cfac * dt;
          if (cnum > best) {
            best      = cnum;
            best_slot = s;
          }
        }
      }
      // sources on the pre-source sums (src/operator.c:663), then the stores
      const int64_t r = (int64_t)m * a.n_owned + o;
      double        bedx, bedy, tbx, tby;
      cell_source<SRC>(a, dt, h, hu, hv, acc1, acc2, dzdx, dzdy, RDY_LD(&t.mannings[r]), bedx, bedy, tbx, tby);
      const double F0 = acc0 + RDY_LD(&t.extsrc[3 * r + 0]);
      const double F1 = acc1 + (-bedx - tbx + RDY_LD(&t.extsrc[3 * r + 1]));
      const double F2 = acc2 + (-bedy - tby + RDY_LD(&t.extsrc[3 * r + 2]));
      if (!EULER || t.f) {
        RDY_ST(&t.f[3 * r + 0], F0);
        RDY_ST(&t.f[3 * r + 1], F1);
        RDY_ST(&t.f[3 * r + 2], F2);
      }
      if (EULER) {
        double *uo = t.u_out + (int64_t)m * t.u_stride;
        RDY_ST(&uo[3 * c + 0], fma(dt, F0, h));
        RDY_ST(&uo[3 * c + 1], fma(dt, F1, hu));
        RDY_ST(&uo[3 * c + 2], fma(dt, F2, hv));
      }
    }
    // the wave's bucket of member m: larger value, then the earlier edge (swe_petsc.c:291 keeps the first).  No barrier.
    const double wmax = wave_max(best);
    int          p    = INT32_MAX;
    if (best > 0.0 && best == wmax) p = pos[(best_slot < 0 ? 0 : best_slot) * a.stride + o];
    p = wave_min(p);
    if (lane == 0) {
      const int64_t b = (int64_t)m * t.n_buckets + bucket;
      t.blk_max[b]    = wmax;
      t.blk_pos[b]    = wmax > 0.0 ? p : -1;
    }
  }
}

// ---- ensembles under hydrostatic reconstruction (rdyhip_ens_hr_enable) -----------------------------------------------------------
// ApplyInteriorFluxHR + the HR source (src/swe/swe_petsc.c:1000-1161, 1229-1263) for every member: ensemble_rhs_kernel's layout,
// grid, member loop, buckets, EnsembleArgs and stores.  What HR needs beyond the plain kernel is GEOMETRY -- the cell's bed
// elevation and its interior neighbours' (KernelArgs::zc_local, which the launch sets) -- loaded once per thread for all members
// of its group, where the bed slopes (which the HR source does not read) were.  Per member, as in tracer_hr_kernel:
//   own cell       two rule sets: riemann_side as it is for the boundary slots and the source (HR is a no-op at boundaries,
//                  operator_fluxes_petsc.c:57-58), the same side after hr_velocity_rule (wet test h > tiny_h, 1061-1064) for the
//                  interior slots; they differ only at h == tiny_h exactly
//   interior slot  the neighbour under riemann_side + hr_velocity_rule, orient_sides, hr_reconstruct with the two elevations in
//                  left / right order, roe_flux on the reconstructed sides.  The edge counts unless both ORIGINAL depths are
//                  below tiny_h (1094); inside that, the flux and the Courant candidate only where a reconstructed depth
//                  exceeds tiny_h (1112) -- a branch: with both at 0 the Roe solver returns 0 / 0 --; then, whenever the outer
//                  guard holds, the own side's pressure correction 0.5 g (h^2 - h_rec^2) (cn, sn) coef (1136-1152)
//   source         cell_source<SRC> with zero bed slopes, as the tiled HR family calls it
template <int S, int SRC, bool EULER>
__global__ __launch_bounds__(BLOCK) void ensemble_hr_kernel(const KernelArgs a, const EnsembleArgs t, const double *__restrict__ u) {
  const int  i      = xcd_block(a.xcd_chunks) * BLOCK + threadIdx.x;
  const bool active = i < a.n_work;
  const int  o      = active ? i : 0;
  const int  lane   = threadIdx.x & 63;

  // ---- the cell's geometry, once for all members of the group
  int32_t id[S], bt[S];
  double  cn[S], sn[S], coef[S];
  int64_t c = 0;
  // The bed elevations -- row S the cell's own, row s its neighbour's through slot s -- wait in LDS, a column per thread (each
  // thread reads back only what it wrote: no barrier), and are read through a volatile pointer where an interior slot needs
  // them.  Held in registers they are loop invariants, and so is everything hr_reconstruct derives from them alone: hipcc then
  // carries zl, zr, max(zl, zr) and two comparison masks per slot across the member loop -- 24 VGPRs and 16 SGPRs with S = 4,
  // which spills SGPRs.
  __shared__ double s_z[S + 1][BLOCK];
  volatile double  *zs = &s_z[0][threadIdx.x];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    id[s] = NBR_EMPTY;
    bt[s] = 0;
    cn[s] = sn[s] = coef[s] = 0.0;
  }
  if (active) {
    const int32_t *nbr = RDY_COLD(a, nbr), *btype = RDY_COLD(a, btype);
    const double  *cn_ = RDY_COLD(a, cn), *sn_ = RDY_COLD(a, sn);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      id[s]   = nbr[s * a.stride + o];
      cn[s]   = cn_[s * a.stride + o];
      sn[s]   = sn_[s * a.stride + o];
      coef[s] = RDY_LD(&a.coef[s * a.stride + o]);
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (id[s] >= 0) zs[s * BLOCK] = a.zc_local[id[s] & NBR_MASK];
      else if (id[s] != NBR_EMPTY) bt[s] = btype[-1 - id[s]];
    }
    c             = a.o2l ? a.o2l[o] : o;
    zs[S * BLOCK] = a.zc_local[c];
  }
  const int32_t *pos    = RDY_COLD(a, pos);
  const int      m0     = blockIdx.y * t.per_group;
  const int      m1     = min(t.n_members, m0 + t.per_group);
  const int      bucket = blockIdx.x * ENSEMBLE_WAVES + (threadIdx.x >> 6);

#pragma unroll 1
  for (int m = m0; m < m1; ++m) {
    const double  dt = t.dts[m];
    const double *um = u + (int64_t)m * t.u_stride;
    double        best      = 0.0;  // largest Courant number of this cell's edges (> 0 only)
    int           best_slot = -1;
    if (active) {
      const double      h    = um[3 * c + 0];
      const double      hu   = um[3 * c + 1];
      const double      hv   = um[3 * c + 2];
      const RiemannSide self = riemann_side(h, hu, hv, a.tiny_h, a.h_anuga_sq);
      RiemannSide       self_hr = self;  // interior edges: the HR operator's own cell
      hr_velocity_rule(self_hr, a.tiny_h);
      double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int32_t nid = id[s];
        if (nid == NBR_EMPTY) continue;  // a triangle in the 4-slot layout, or an outer edge that belongs to no boundary
        const double cfac = fabs(coef[s]);  // len / area_self: the max over an edge's two cells is len / min(area_l, area_r)
        if (nid >= 0) {
          const int64_t n     = nid & NBR_MASK;
          RiemannSide   other = riemann_side(um[3 * n + 0], um[3 * n + 1], um[3 * n + 2], a.tiny_h, a.h_anuga_sq);
          hr_velocity_rule(other, a.tiny_h);
          const bool  self_left = coef[s] < 0.0;
          RiemannSide L, R, Lr, Rr;
          orient_sides(self_hr, other, self_left, L, R);
          const double z_self = zs[S * BLOCK], z_nbr = zs[s * BLOCK];
          hr_reconstruct(L, R, self_left ? z_self : z_nbr, self_left ? z_nbr : z_self, Lr, Rr);
          const RoeFlux fl = roe_flux(Lr, Rr, sn[s], cn[s]);
          if (!(R.h < a.tiny_h && L.h < a.tiny_h)) {
            if (Lr.h > a.tiny_h || Rr.h > a.tiny_h) {
              acc0 += fl.f0 * coef[s];
              acc1 += fl.f1 * coef[s];
              acc2 += fl.f2 * coef[s];
              const double cnum = fl.amax * cfac * dt;
              if (cnum > best) {
                best      = cnum;
                best_slot = s;
              }
            }
            const double h_rec = self_left ? Lr.h : Rr.h;
            const double corr  = 0.5 * GRAVITY * (h * h - h_rec * h_rec);
            acc1 += corr * cn[s] * coef[s];
            acc2 += corr * sn[s] * coef[s];
          }
        } else {
          const int64_t      k  = (int64_t)m * t.k_stride + 3 * (int64_t)(-1 - nid);
          const BoundaryFlux bf = boundary_flux(bt[s], true, self, t.bvalues + k, sn[s], cn[s], a.tiny_h, a.h_anuga_sq);
          t.bflux[k + 0]        = bf.flux.f0;  // boundary_fluxes[b], swe_petsc.c:574
          t.bflux[k + 1]        = bf.flux.f1;
          t.bflux[k + 2]        = bf.flux.f2;
          if (bf.wet) {
            acc0 += bf.flux.f0 * coef[s];
            acc1 += bf.flux.f1 * coef[s];
            acc2 += bf.flux.f2 * coef[s];
            const double cnum = bf.flux.amax * cfac * dt;
            if (cnum > best) {
              best      = cnum;
              best_slot = s;
            }
          }
        }
      }
      // sources on the pre-source sums (src/operator.c:663) without the bed slope, then the stores
      const int64_t r = (int64_t)m * a.n_owned + o;
      double        bedx, bedy, tbx, tby;
      cell_source<SRC>(a, dt, h, hu, hv, acc1, acc2, 0.0, 0.0, RDY_LD(&t.mannings[r]), bedx, bedy, tbx, tby);
      const double F0 = acc0 + RDY_LD(&t.extsrc[3 * r + 0]);
      const double F1 = acc1 + (-bedx - tbx + RDY_LD(&t.extsrc[3 * r + 1]));
      const double F2 = acc2 + (-bedy - tby + RDY_LD(&t.extsrc[3 * r + 2]));
      if (!EULER || t.f) {
        RDY_ST(&t.f[3 * r + 0], F0);
        RDY_ST(&t.f[3 * r + 1], F1);
        RDY_ST(&t.f[3 * r + 2], F2);
      }
      if (EULER) {
        double *uo = t.u_out + (int64_t)m * t.u_stride;
        RDY_ST(&uo[3 * c + 0], fma(dt, F0, h));
        RDY_ST(&uo[3 * c + 1], fma(dt, F1, hu));
        RDY_ST(&uo[3 * c + 2], fma(dt, F2, hv));
      }
    }
    // the wave's bucket of member m: larger value, then the earlier edge (swe_petsc.c:291 keeps the first).  No barrier.
    const double wmax = wave_max(best);
    int          p    = INT32_MAX;
    if (best > 0.0 && best == wmax) p = pos[(best_slot < 0 ? 0 : best_slot) * a.stride + o];
    p = wave_min(p);
    if (lane == 0) {
      const int64_t b = (int64_t)m * t.n_buckets + bucket;
      t.blk_max[b]    = wmax;
      t.blk_pos[b]    = wmax > 0.0 ? p : -1;
    }
  }
}

// Merges every member's buckets into its 16-byte diagnostic: workgroup m = member m (rdyhip_ensemble_update_diagnostics)
__global__ __launch_bounds__(BLOCK) void ensemble_courant_finalize_kernel(int n_buckets, const double *__restrict__ blk_max,
                                                                         const int32_t *__restrict__ blk_pos, DeviceCourant *diag) {
  const int64_t base = (int64_t)blockIdx.x * n_buckets;
  double        m    = 0.0;
  int           p    = INT32_MAX;
  for (int i = threadIdx.x; i < n_buckets; i += BLOCK) {
    const double v = blk_max[base + i];
    const int    q = blk_pos[base + i];
    if (v > m || (v == m && v > 0.0 && q < p)) {
      m = v;
      p = q;
    }
  }
  __shared__ double s_max[ENSEMBLE_WAVES];
  __shared__ int    s_pos[ENSEMBLE_WAVES];
  const int    lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double wm = wave_max(m);
  int          wp = (m == wm && m > 0.0) ? p : INT32_MAX;
  wp              = wave_min(wp);
  if (lane == 0) {
    s_max[wave] = wm;
    s_pos[wave] = wp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double bm = 0.0;
    int    bp = INT32_MAX;
    for (int w = 0; w < ENSEMBLE_WAVES; ++w) {
      if (s_max[w] > bm || (s_max[w] == bm && bm > 0.0 && s_pos[w] < bp)) {
        bm = s_max[w];
        bp = s_pos[w];
      }
    }
    diag[blockIdx.x].max_courant = bm;
    diag[blockIdx.x].pos         = bm > 0.0 ? bp : -1;
  }
}

}  // namespace rdyhip
