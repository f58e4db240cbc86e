// MI355X-native SWE right-hand-side operator: the one translation unit of the library.  Here: create / destroy, the launch
// selection and the thin entry points of the C ABI declared in include/rdyhip.h; the mesh repack is host_layout.h, the
// operator's state operator_state.h, the setters field_io.h, the ghost exchange halo_*.h.  gfx950 only.
//
// Layout (built by host_layout.h): one thread owns one owned cell.  The cell's
// edges are stored as up to S "slots" (S = 3 for triangle meshes, 4 when
// quads are present), struct-of-arrays by slot so that every per-slot array
// is read with unit stride across a wavefront:
//     nbr [s][o]  int32   neighbour's local cell id (| NBR_GHOST), or -1-k for
//                         boundary edge k, or NBR_EMPTY
//     cn,sn[s][o] double  the edge's unit normal in its canonical left->right
//                         orientation (edges.cn/sn)
//     coef[s][o]  double  -len/area_self if this cell is the edge's left cell,
//                         +len/area_self if it is the right cell -- the factor
//                         the reference multiplies the edge flux by
//                         (src/swe/swe_petsc.c:301-305); its sign is the
//                         orientation flag
// Slots are ordered by the position of the edge in the reference's loops
// (internal edges in internal_edge_ids order, then boundary 0's edges, ...),
// so a cell's contributions are summed in the reference's order.  Each edge
// flux is evaluated in the canonical orientation from both of its cells, so
// the two evaluations are bitwise equal and the scheme stays conservative
// without atomics or a scatter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "rdyhip.h"
#include "error.h"
#include "tile_format.h"
#include "host_layout.h"
#include "swe_device.h"
#include "swe_kernels.h"
#include "forcing_kernels.h"
#include "muscl_kernels.h"
#include "rk_kernels.h"
#include "output_kernels.h"
#include "series_plan.h"
#include "series_kernels.h"
#include "readout_kernels.h"
#include "tracer_kernels.h"
#include "ensemble_kernels.h"
#include "operator_state.h"

using namespace rdyhip;


namespace {

using TiledKernelFn = void (*)(const KernelArgs, const double, const double *, double *);

void halo_forget_packed_state(RDyHipHalo_s *h);   // halo_exchange.h
void halo_operator_gone(RDyHipHalo_s *h);

// std::true_type / std::false_type for a run-time flag: how the two selectors below turn a launch's choices into template arguments
template <class F>
auto with_flag(bool b, F f) {
  return b ? f(std::true_type()) : f(std::false_type());
}

// The instantiation of the tiled kernel for (slots per cell, source method, f = rhs (else f += rhs), HR, the forward-Euler update
// fused into the stores (rdyhip_euler_step; always f = rhs), F -- Euler step: u_out -- stored with the non-temporal hint)
TiledKernelFn tiled_kernel_fn(int S, int src, bool ovw, bool hr, bool euler, bool fnt) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(src != 0, [&](auto xq) { return with_flag(hr, [&](auto hr_) {
    return with_flag(fnt, [&](auto nt) -> TiledKernelFn {
      constexpr int s = quad ? 4 : 3, x = xq ? 1 : 0;
      if (euler) return swe_rhs_tiled_kernel<s, x, true, hr_, true, nt>;
      return ovw ? swe_rhs_tiled_kernel<s, x, true, hr_, false, nt> : swe_rhs_tiled_kernel<s, x, false, hr_, false, nt>;
    });
  }); }); });
}

using MusclKernelFn = void (*)(const KernelArgs, const MusclArgs, const double, const double *, double *);

// The instantiation of the second-order kernel for (slots per cell, source method, f = rhs, the fused Euler step, limiter)
MusclKernelFn muscl_kernel_fn(int S, int src, bool ovw, bool euler, int limiter) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(src != 0, [&](auto xq) {
    auto form = [&](auto lim) -> MusclKernelFn {
      constexpr int s = quad ? 4 : 3, x = xq ? 1 : 0;
      if (euler) return swe_rhs_muscl_fused_kernel<s, x, true, lim, true>;
      return ovw ? swe_rhs_muscl_fused_kernel<s, x, true, lim, false> : swe_rhs_muscl_fused_kernel<s, x, false, lim, false>;
    };
    switch (limiter) {
      case RDYHIP_LIMITER_NONE: return form(std::integral_constant<int, LIMITER_NONE>());
      case RDYHIP_LIMITER_VANLEER: return form(std::integral_constant<int, LIMITER_VANLEER>());
      default: return form(std::integral_constant<int, LIMITER_MINMOD>());
    }
  }); });
}

MusclArgs muscl_args(RDyHipOperator op) {
  MusclArgs g{};
  g.grad  = op->d_grad.p;
  g.e_mid = op->d_e_mid.p;
  g.cxy   = op->d_cxy.p;
  g.hcells2 = op->d_hcells2.p;
  g.r2_off  = op->d_c_off.p;
  g.bn_idx  = op->d_bn_idx.p;
  return g;
}

// A launch of one thread per owned cell (cell-centric kernel, gradient kernel): the halo cell list, or all owned cells in
// XCD chunks.  Sets the work of `a`, returns the grid.
int cell_launch_work(RDyHipOperator op, int32_t phase, KernelArgs &a) {
  if (phase == RDYHIP_PHASE_HALO) {
    a.list       = op->d_halo_list.p;
    a.n_work     = op->n_halo;
    a.xcd_chunks = 0;
    a.phase      = RDYHIP_PHASE_ALL;  // the list already holds exactly the halo cells
    return (op->n_halo + BLOCK - 1) / BLOCK;
  }
  a.list       = nullptr;
  a.n_work     = op->n_owned;
  a.xcd_chunks = op->xcd_chunks;
  return op->grid;
}

// ComputeLeastSquaresGradients for the owned cells selected by `phase`
int launch_gradients(RDyHipOperator op, int32_t phase, const double *u, hipStream_t st) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (!op->muscl) return fail(RDYHIP_ERR_USER, "the operator was not created with second_order");
  if (phase != RDYHIP_PHASE_ALL && phase != RDYHIP_PHASE_INTERIOR && phase != RDYHIP_PHASE_HALO) return fail(RDYHIP_ERR_USER, "unknown phase %d", phase);
  if (op->n_owned == 0) return 0;
  if (!u) return fail(RDYHIP_ERR_USER, "null u_local");
  KernelArgs a{};
  a.n_owned = op->n_owned;
  a.stride  = op->stride;
  a.o2l     = op->prefix ? nullptr : op->d_o2l.p;
  a.cold    = op->d_cold.p;
  a.phase   = phase;
  if (phase == RDYHIP_PHASE_HALO) {
    if (op->n_halo == 0) return 0;
    // with a fused pack attached this launch stores gradient rows into the halo's send buffer (ColdArgs::gsend_*):
    // whatever state rows it mirrored are gone
    if (op->fused_halo) halo_forget_packed_state(op->fused_halo);
  }
  const int grid = cell_launch_work(op, phase, a);
  const MusclArgs g = muscl_args(op);
  if (op->S == 3) hipLaunchKernelGGL((muscl_gradient_kernel<3>), dim3(grid), dim3(BLOCK), 0, st, a, g, u);
  else hipLaunchKernelGGL((muscl_gradient_kernel<4>), dim3(grid), dim3(BLOCK), 0, st, a, g, u);
  HIP_TRY(hipGetLastError());
  return 0;
}

// bucket_half: which of the Courant buckets (one per workgroup, merged on demand) the launch owns -- 0: all of them (every
// ordinary launch); 1 / 2: the first / second half, for the interior and the halo launch of rdyhip_rhs_overlapped, which
// run side by side on two streams and must not share a bucket
int launch_rhs(RDyHipOperator op, int32_t phase, int32_t overwrite, int reset_diag, double dt, const double *u, double *f, hipStream_t st,
               bool gradients_ready = false, double *u_out = nullptr, int bucket_half = 0, const hipStream_t *joined_on = nullptr) {
  // joined_on: the caller's stream, where `st` is the library's exchange stream (the halo launch of a two-stream step)
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  // an Euler-step launch rewrites the attached halo's send buffer (tiles flagged TILE_SEND_FLAG): whatever it held is gone
  // (rdyhip_euler_step_overlapped notes the new content itself once its launches are enqueued)
  if (u_out && op->fused_halo) halo_forget_packed_state(op->fused_halo);
  // rdyhip_euler_step: the tiled kernels have the update fused into their stores (F optional); the cell-centric
  // kernel evaluates F (into a scratch vector if the caller wants none) and a separate update follows
  const bool euler_fused = u_out && op->use_tiled;
  if (u_out && !euler_fused && !f && op->n_owned > 0) {
    if (!op->d_scratch_f.p) {
      int rc = op->d_scratch_f.alloc((size_t)3 * op->n_owned);
      if (rc) return rc;
    }
    f = op->d_scratch_f.p;
  }
  if (op->muscl && !gradients_ready && op->n_owned > 0) {
    // only ghost cells' gradients are read from memory, and they have to come from the exchange (CommunicateCellGradients):
    // rdyhip_compute_gradients(RDYHIP_PHASE_HALO), exchange of the ghost rows, then RDYHIP_PHASE_GRADIENTS_READY
    if (op->n_cells > op->n_owned || phase != RDYHIP_PHASE_ALL)
      return fail(RDYHIP_ERR_USER, "second_order with ghost cells or a phased apply needs RDYHIP_PHASE_GRADIENTS_READY (see rdyhip_compute_gradients)");
  }
  if (op->n_owned == 0) return reset_diag ? rdyhip_reset_diagnostics(op, (void *)st) : 0;  // a rank may own nothing (f_global is then empty)
  if (!u || (!f && !euler_fused)) return fail(RDYHIP_ERR_USER, "null u_local / f_global");
  KernelArgs a{};
  a.u_out      = u_out;
  a.n_owned    = op->n_owned;
  a.stride     = op->stride;
  a.o2l        = op->prefix ? nullptr : op->d_o2l.p;
  a.cold       = op->d_cold.p;
  a.coef       = op->d_coef.p;
  a.dzdx       = op->d_dzdx.p;
  a.dzdy       = op->d_dzdy.p;
  a.mannings   = op->d_mannings.p;
  a.extsrc     = op->d_extsrc.p;
  a.src_mom    = 1;
  // read here, when the launch is enqueued (like src_water_only below).  Not stored: the request that comes later derives
  // them from this launch's input state, on the stream the caller ordered it on
  a.pv         = op->pv_wanted ? op->d_pv.p : nullptr;
  if (!a.pv) {
    op->pv_pending = true;
    op->pv_u       = u;
    op->pv_stream  = joined_on ? *joined_on : st;
  }
  a.fdiv       = op->keep_fdiv ? op->d_fdiv.p : nullptr;
  a.n_buckets  = (int32_t)op->d_blk_max.n;
  a.bucket_off = 0;
  if (bucket_half) {
    const int32_t half = a.n_buckets / 2;
    a.n_buckets = half;
    if (bucket_half == 2) a.bucket_off = half;
  }
  a.reset_diag = reset_diag ? 1 : 0;
  a.tiny_h     = op->config.tiny_h;
  a.h_anuga_sq = op->config.h_anuga_regular * op->config.h_anuga_regular;
  a.xq_thresh  = op->config.xq2018_threshold;
  a.overwrite  = overwrite ? 1 : 0;
  a.phase      = phase;

  a.tiles    = op->d_tiles.p;
  a.e_lr     = op->d_e_lr.p;
  a.e_cs     = op->d_e_cs.p;
  a.hcells   = op->d_hcells.p;
  a.slot_ref = op->S == 3 ? (const void *)op->d_slot_ref3.p : (const void *)op->d_slot_ref.p;
  a.zc_local = op->d_zc_local.p;

  int        grid = 0;
  const bool xq = op->config.source_method == RDYHIP_SOURCE_IMPLICIT_XQ2018;
  // a HALO phase on a rank without ghost-adjacent cells has no flux launch, but the tail below (boundary edges of
  // ghost cells, the separate Euler update of the non-fused kernels) still belongs to it
  const bool nothing_to_launch = phase == RDYHIP_PHASE_HALO && (op->use_tiled ? op->n_halo_tiles == 0 : op->n_halo == 0);
  if (nothing_to_launch) {
  } else if (op->use_tiled) {
    const int pgrid = op->muscl ? op->pgrid_muscl : op->pgrid;
    // persistent workgroups: at most as many as the device holds at once
    if (phase == RDYHIP_PHASE_HALO) {
      a.list       = op->d_halo_tiles.p;
      a.n_work     = op->n_halo_tiles;
      a.xcd_chunks = 0;
      a.phase      = RDYHIP_PHASE_ALL;  // the list already holds exactly the halo tiles
      grid         = std::min(pgrid, op->n_halo_tiles);
    } else {
      a.list   = nullptr;
      a.n_work = op->ntiles;
      // While the interior phase runs, the halo exchange's pack / RCCL / unpack kernels need somewhere
      // to run: the persistent grid would otherwise fill every SIMD's register file for the whole launch.
      const int shrink = phase == RDYHIP_PHASE_INTERIOR ? op->interior_shrink : 0;
      const int pg     = shrink > 0 ? std::max(8, pgrid - std::max(8, pgrid / shrink)) : pgrid;
      if (op->tiled_xcd_chunks > 0) {
        a.xcd_chunks = op->tiled_xcd_chunks;
        int per_xcd  = std::max(1, std::min(pg >> 3, op->tiled_xcd_chunks));
        if (op->balance_rounds) {
          // every workgroup of an XCD walks the same number of tiles (+-1): a mesh of 3 907 tiles on 768 resident workgroups
          // would otherwise run five full rounds and a sixth with 9 % of the device busy
          const int rounds = (op->tiled_xcd_chunks + per_xcd - 1) / per_xcd;
          per_xcd          = (op->tiled_xcd_chunks + rounds - 1) / rounds;
        }
        grid = per_xcd * 8;
      } else {
        a.xcd_chunks = 0;
        grid         = std::min(pg, op->ntiles);
      }
    }
    if (op->muscl) {
      MusclKernelFn kfn = muscl_kernel_fn(op->S, xq ? 1 : 0, overwrite != 0, euler_fused, op->config.limiter);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(grid), dim3(TILE), op->lds_muscl, st, a, muscl_args(op), dt, u, f);
    } else {
      // plain (cached) stores: of u_out for states that fit the Infinity Cache, of F under RDYHIP_CONFIG_CACHED_F_STORES
      const bool     cached = euler_fused ? op->uout_cached : (op->config.flags & RDYHIP_CONFIG_CACHED_F_STORES) != 0;
      TiledKernelFn  kfn    = tiled_kernel_fn(op->S, xq ? 1 : 0, overwrite != 0, op->hr, euler_fused, !cached);
      // the flag is read here, when the launch is enqueued: launches and source writers on one stream stay consistent
      if (op->src_water_only) {
        a.extsrc  = op->d_src_water.p;
        a.src_mom = 0;
      }
      // ... and so are the uniform fields: UNIFORM_* bit i is STREAM_* bit i + 1 (element 0 of each array is the value, kept
      // current on the stream by the setters: nothing but these bits goes to the kernel)
      a.src_mom |= op->uniform.mask(op->src_water_only) << 1;
      // The dynamic walk: whole-mesh launches over XCD chunks.  INTERIOR launches skip tiles (their draws would run in
      // series) and HALO launches walk a list: both keep the static walk, and neither touches the counters, so they may
      // run beside each other as before.  PHASE_ALL launches of one operator already follow each other (the Courant buckets).
      // Default: from TILE_WALK_MIN_ROUNDS tiles per workgroup.  Measured at 38 (10 M triangles: 6.5 % faster) and at 3.8
      // (1 M: 13 % slower, three of the four tiles are the static ones anyway); not swept between (RESULTS_LOG section 21).
      const bool dyn_ok   = tiled_has_dynamic_walk(op->S, xq ? 1 : 0, op->hr, euler_fused) && phase == RDYHIP_PHASE_ALL && a.xcd_chunks > 0 && !a.list;
      const bool dyn_want = op->tile_walk >= 0 ? op->tile_walk == 1 : (int64_t)a.xcd_chunks * 8 >= (int64_t)TILE_WALK_MIN_ROUNDS * grid;
      a.tile_walk = dyn_ok && dyn_want ? TILE_WALK_DYNAMIC
                    : a.phase == RDYHIP_PHASE_INTERIOR                                                ? TILE_WALK_STATIC_SKIP
                                                                                                       : TILE_WALK_STATIC;
      hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(grid), dim3(TILE), op->lds_bytes, st, a, dt, u, f);
    }
  } else {
    grid = cell_launch_work(op, phase, a);
    if (op->S == 3) {
      if (xq) hipLaunchKernelGGL((swe_rhs_kernel<3, 1>), dim3(grid), dim3(BLOCK), 0, st, a, dt, u, f);
      else hipLaunchKernelGGL((swe_rhs_kernel<3, 0>), dim3(grid), dim3(BLOCK), 0, st, a, dt, u, f);
    } else {
      if (xq) hipLaunchKernelGGL((swe_rhs_kernel<4, 1>), dim3(grid), dim3(BLOCK), 0, st, a, dt, u, f);
      else hipLaunchKernelGGL((swe_rhs_kernel<4, 0>), dim3(grid), dim3(BLOCK), 0, st, a, dt, u, f);
    }
  }
  HIP_TRY(hipGetLastError());
  // boundary edges hanging off ghost cells (diagnostic vectors only); once per full apply
  if (op->n_bghost > 0 && phase != RDYHIP_PHASE_INTERIOR) {
    hipLaunchKernelGGL(boundary_ghost_kernel, dim3((op->n_bghost + 63) / 64), dim3(64), 0, st, op->n_bghost, op->d_bghost_list.p, op->d_bleft.p,
                       op->d_btype.p, op->d_bcn.p, op->d_bsn.p, op->d_bvalues.p, op->d_bflux.p, op->d_baccum.p, u, dt, a.tiny_h, a.h_anuga_sq);
    HIP_TRY(hipGetLastError());
  }
  if (u_out && !euler_fused && phase != RDYHIP_PHASE_INTERIOR) {
    // F is complete once the halo (or the only) phase has run
    const int64_t n3 = 3 * (int64_t)op->n_owned;
    hipLaunchKernelGGL(euler_out_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, op->n_owned, op->prefix ? nullptr : op->d_o2l.p, dt, f, u, u_out);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace

#include "field_io.h"

extern "C" {

const char *rdyhip_last_error(void) { return g_err.c_str(); }
int32_t     rdyhip_version(void) { return RDYHIP_VERSION; }

int rdyhip_create(const RDyHipConfig *config, const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries,
                  RDyHipOperator *op_out) {
  if (!config || !mesh || !op_out) return fail(RDYHIP_ERR_USER, "null argument to rdyhip_create");
  *op_out = nullptr;
  HostLayout L;
  int        rc = build_host_layout(config, mesh, num_boundaries, boundaries, L);
  if (rc) return rc;

  // ---- build the operator --------------------------------------------------
  std::unique_ptr<RDyHipOperator_s> op(new (std::nothrow) RDyHipOperator_s);
  if (!op) return fail(RDYHIP_ERR_MEM, "out of host memory");
  static_cast<LayoutCounts &>(*op) = L.counts;
  op->config     = *config;
  op->n_internal = L.ni;
  op->stride     = L.stride;
  op->n_bghost   = (int32_t)L.bghost.size();
  op->n_xedges   = (int32_t)L.x_pos.size();
  op->hr         = L.hr_on;
  const int32_t S = L.S, ntiles = L.ntiles;
  const int     xq = config->source_method == RDYHIP_SOURCE_IMPLICIT_XQ2018 ? 1 : 0;
  {
    // The Euler-step kernels' u_out is what the next step reads: stored without the non-temporal hint it is still in the
    // Infinity Cache (256 MB) then -- when it fits beside what else lives there.  A sweep over 0.36 M .. 10 M cells in a time loop
    // (profiles/r05_uout_policy_sweep.txt): plain stores win 3-5 % from 1.2 M to 6 M cells (29 .. 150 MB of state), lose 0.3-3 %
    // below 1 M (the launch is over before a second pass could profit) and 2 % from 8 M cells.  So: plain stores for
    // 28 MB <= state <= 144 MB; RDYHIP_UOUT_CACHED=0 / 1 forces.  (The upper bound had a knob of its own while it was swept; the
    // sweep itself only ever forced the policy, and the library keeps to sixteen environment variables.)
    const double max_mb = 144.0;
    const double state_bytes = 24.0 * (double)op->n_cells;
    op->uout_cached = state_bytes >= 28.0 * 1048576.0 && state_bytes <= max_mb * 1048576.0;
    if (const char *e = getenv("RDYHIP_UOUT_CACHED")) op->uout_cached = atoi(e) != 0;
  }
  {
    const char *kenv = getenv("RDYHIP_KERNEL");
    op->use_tiled    = !(kenv && strcmp(kenv, "cell") == 0);
    if ((op->hr || op->muscl) && !op->use_tiled)
      return fail(RDYHIP_ERR_USER, "hydrostatic reconstruction and second_order are implemented by the tiled kernels only (unset RDYHIP_KERNEL=cell)");
  }
  if (hipGetDevice(&op->device) != hipSuccess) return fail(RDYHIP_ERR_LIB, "hipGetDevice failed: no usable HIP device");

  const int tiles_n = (op->n_owned + BLOCK - 1) / BLOCK;
  const char *env   = getenv("RDYHIP_XCD_SWIZZLE");
  const bool  swz   = env ? atoi(env) != 0 : true;
  op->xcd_chunks    = (swz && tiles_n >= 64) ? (tiles_n + 7) / 8 : 0;
  op->grid          = op->xcd_chunks > 0 ? op->xcd_chunks * 8 : tiles_n;
  {
    // size of the persistent grid: resident workgroups per CU (occupancy query) x CUs
    int cus = 256, per_cu = 4, per_cu_forced = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, op->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    if (const char *e2 = getenv("RDYHIP_BLOCKS_PER_CU")) per_cu_forced = atoi(e2);
    int q = 0;
    const void *kfn = (const void *)tiled_kernel_fn(S, xq, true, op->hr, false, true);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kfn, TILE, op->lds_bytes) == hipSuccess && q > 0) per_cu = q;
    // the family's own setting (tiled_blocks_per_cu): a kernel compiled for three waves per SIMD may well fit four
    per_cu = std::min(per_cu, tiled_blocks_per_cu(S, xq, op->hr));
    if (per_cu_forced > 0) per_cu = per_cu_forced;
    op->pgrid            = std::max(8, cus * per_cu);
    if (op->muscl) {
      int qm = 0, per_cu_m = 2;
      const void *mfn = (const void *)muscl_kernel_fn(S, xq, true, false, config->limiter);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&qm, mfn, TILE, op->lds_muscl) == hipSuccess && qm > 0) per_cu_m = qm;
      if (per_cu_forced > 0) per_cu_m = per_cu_forced;
      op->pgrid_muscl = std::max(8, cus * per_cu_m);
    }
    op->tiled_xcd_chunks = (swz && ntiles >= 64) ? (ntiles + 7) / 8 : 0;
    if (const char *e3 = getenv("RDYHIP_INTERIOR_SHRINK")) op->interior_shrink = std::max(0, atoi(e3));  // measurement knob
    if (const char *e4 = getenv("RDYHIP_PGRID")) {  // measurement knob: the persistent grid itself
      if (atoi(e4) >= 8) op->pgrid = op->pgrid_muscl = atoi(e4) & ~7;
    }
    if (const char *e5 = getenv("RDYHIP_BALANCE_ROUNDS")) op->balance_rounds = atoi(e5) != 0;  // moot under the dynamic walk
    if (const char *e6 = getenv("RDYHIP_TILE_WALK")) {
      if (strcmp(e6, "static") != 0 && strcmp(e6, "dynamic") != 0) return fail(RDYHIP_ERR_USER, "RDYHIP_TILE_WALK is 'static' or 'dynamic', not '%s'", e6);
      op->tile_walk = strcmp(e6, "dynamic") == 0 ? 1 : 0;
    }
  }
  const int    maxgrid = std::max(std::max(std::max(op->grid, op->pgrid), op->pgrid_muscl), 1);
  const size_t no = (size_t)op->n_owned, nc = (size_t)op->n_cells, K = (size_t)op->K;

  if (!L.prefix) rc = op->d_o2l.upload(L.o2l);
  if (!rc) rc = op->d_nbr.upload(L.nbr);
  if (!rc) rc = op->d_pos.upload(L.pos);
  if (!rc) rc = op->d_cn.upload(L.cn);
  if (!rc) rc = op->d_sn.upload(L.sn);
  if (!rc) rc = op->d_coef.upload(L.coef);
  if (!rc) rc = op->d_dzdx.upload(L.dzdx);
  if (!rc) rc = op->d_dzdy.upload(L.dzdy);
  if (!rc) rc = op->d_halo_list.upload(L.halo);
  if (!rc) rc = op->d_btype.upload(L.btype);
  if (!rc) rc = op->d_bleft.upload(L.bleft);
  if (!rc) rc = op->d_bghost_list.upload(L.bghost);
  if (!rc) rc = op->d_bcn.upload(L.bcn);
  if (!rc) rc = op->d_bsn.upload(L.bsn);
  if (!rc) rc = op->d_tiles.upload(L.tiles);
  if (!rc) rc = op->d_halo_tiles.upload(L.halo_tiles);
  if (!rc) rc = op->d_e_lr.upload(L.e_lr);
  if (!rc) rc = op->d_e_pos.upload(L.e_pos);
  if (!rc) rc = op->d_x_lr.upload(L.x_lr);
  if (!rc) rc = op->d_x_flags.upload(L.x_flags);
  if (!rc) rc = op->d_x_cs.upload(L.x_cs);
  if (!rc) rc = op->d_x_cfac.upload(L.x_cfac);
  if (!rc) rc = op->d_x_mid.upload(L.x_mid);
  if (!rc) rc = op->d_hcells.upload(L.hcells);
  if (!rc) rc = op->d_tile_bk.upload(L.tile_bk);
  if (!rc) rc = op->d_tile_boff.upload(L.tile_boff);
  if (!rc) rc = op->d_e_cs.upload(L.e_cs);
  if (!rc) rc = S == 3 ? op->d_slot_ref3.upload(L.ref3) : op->d_slot_ref.upload(L.slot_ref);
  if (!rc && op->hr) rc = op->d_zc_local.upload(L.zc);
  if (op->muscl) {
    if (!rc) rc = op->d_grad.zeros(6 * nc);
    if (!rc) rc = op->d_e_mid.upload(L.e_mid);
    if (!rc) rc = op->d_cxy.upload(L.cxy);
    if (!rc) rc = op->d_hcells2.upload(L.hcells2);
    if (!rc) rc = op->d_c_off.upload(L.c_off);
    if (!rc) rc = op->d_bn_idx.upload(L.bn_idx);
  }
  if (!rc) rc = op->d_mannings.zeros(no);
  if (!rc) rc = op->d_extsrc.zeros(3 * no);
  if (!rc) rc = op->d_src_water.zeros(no);
  {
    const char *e = getenv("RDYHIP_UNIFORM_FIELDS");   // the A/B and test knob
    op->uniform.start(!(e && atoi(e) == 0), bed_is_flat(L.dzdx.data(), L.dzdy.data(), (int64_t)std::min(L.dzdx.size(), L.dzdy.size())));
  }
  if (!rc) rc = op->d_bvalues.zeros(3 * K);
  if (!rc) rc = op->d_bflux.zeros(3 * K);
  if (!rc) rc = op->d_baccum.zeros(3 * K);
  if (!rc) rc = op->d_pv.zeros(3 * no);
  if (!rc) rc = op->d_blk_max.zeros((size_t)2 * maxgrid);  // two halves: see launch_rhs(bucket_half)
  if (!rc) rc = op->d_blk_pos.zeros((size_t)2 * maxgrid);
  if (!rc) rc = op->d_courant.zeros(1);
  if (!rc) rc = op->d_tile_draw.zeros(9 * TILE_DRAW_STRIDE);
  if (!rc) {
    ColdArgs c{};
    c.nbr = op->d_nbr.p; c.cn = op->d_cn.p; c.sn = op->d_sn.p; c.pos = op->d_pos.p; c.e_pos = op->d_e_pos.p;
    c.btype = op->d_btype.p; c.bvalues = op->d_bvalues.p; c.bflux = op->d_bflux.p; c.baccum = op->d_baccum.p;
    c.tile_bk = op->d_tile_bk.p; c.tile_boff = op->d_tile_boff.p;
    c.n_xedges = op->n_xedges; c.x_rec0 = (int32_t)L.e_lr.size(); c.x_lr = op->d_x_lr.p; c.x_flags = op->d_x_flags.p; c.x_cs = op->d_x_cs.p;
    c.x_cfac = op->d_x_cfac.p; c.x_mid = op->d_x_mid.p;
    c.blk_max = op->d_blk_max.p; c.blk_pos = op->d_blk_pos.p;
    c.tile_draw = op->d_tile_draw.p;
    rc = op->d_cold.upload(std::vector<ColdArgs>(1, c));
  }
  if (rc) return rc;
  hipLaunchKernelGGL(courant_reset_kernel, dim3(4), dim3(1024), 0, 0, (int)op->d_blk_max.n, op->d_blk_max.p, op->d_blk_pos.p);
  if (hipDeviceSynchronize() != hipSuccess) return fail(RDYHIP_ERR_LIB, "device synchronisation failed after create");

  // host copies: what resolves the Courant position into ids, and what the halo's send lists are built from
  op->h_area.assign(mesh->cell_areas, mesh->cell_areas + nc);
  op->h_internal_edge.assign(mesh->edge_internal_ids, mesh->edge_internal_ids + L.ni);
  op->h_edge_cells.assign(mesh->edge_cell_ids, mesh->edge_cell_ids + 2 * (size_t)L.ne);
  op->h_blen.resize(K);   // the record plan of the boundary-flux series needs them after the mesh pointers are gone
  for (size_t k = 0; k < K; ++k) op->h_blen[k] = mesh->edge_lengths[L.bedge[k]];
  op->h_bghost  = std::move(L.bghost);
  op->h_bedge   = std::move(L.bedge);
  op->h_btype   = std::move(L.btype);
  op->h_boff    = std::move(L.boff);
  op->h_tile_c0 = std::move(L.tile_c0);
  if (!L.prefix) op->h_l2o.assign(mesh->cell_local_to_owned, mesh->cell_local_to_owned + nc);
  if (mesh->cell_global_ids) op->h_cell_gid.assign(mesh->cell_global_ids, mesh->cell_global_ids + nc);
  if (mesh->edge_global_ids) op->h_edge_gid.assign(mesh->edge_global_ids, mesh->edge_global_ids + L.ne);

  op->device_bytes = op->d_o2l.bytes() + op->d_nbr.bytes() + op->d_pos.bytes() + op->d_cn.bytes() + op->d_sn.bytes() + op->d_coef.bytes() +
                     op->d_dzdx.bytes() + op->d_dzdy.bytes() + op->d_mannings.bytes() + op->d_extsrc.bytes() + op->d_src_water.bytes() +
                     op->d_pv.bytes() + op->d_bvalues.bytes() + op->d_bflux.bytes() + op->d_baccum.bytes() + op->d_blk_max.bytes() +
                     op->d_blk_pos.bytes() + op->d_tiles.bytes() + op->d_e_lr.bytes() + op->d_e_pos.bytes() + op->d_hcells.bytes() + op->d_tile_bk.bytes() + op->d_tile_boff.bytes() +
                     op->d_e_cs.bytes() + op->d_slot_ref.bytes() + op->d_slot_ref3.bytes() + op->d_grad.bytes() + op->d_e_mid.bytes() +
                     op->d_cxy.bytes() + op->d_hcells2.bytes() + op->d_c_off.bytes() + op->d_bn_idx.bytes();
  *op_out = op.release();
  return 0;
}

int rdyhip_destroy(RDyHipOperator *op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null argument to rdyhip_destroy");
  if (*op) {
    (void)hipDeviceSynchronize();
    if ((*op)->fused_halo) halo_operator_gone((*op)->fused_halo);
    delete *op;
    *op = nullptr;
  }
  return 0;
}

int rdyhip_apply(RDyHipOperator op, double dt, const double *u_local, double *f_global, void *stream) {
  return launch_rhs(op, RDYHIP_PHASE_ALL, 0, 0, dt, u_local, f_global, (hipStream_t)stream);
}

int rdyhip_rhs_function(RDyHipOperator op, double dt, const double *u_local, double *f_global, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  op->courant = RDyHipCourant{0.0, -1, -1};
  // the diagnostic reset rides on the Courant finalize kernel (no extra launch)
  return launch_rhs(op, RDYHIP_PHASE_ALL, 1, 1, dt, u_local, f_global, (hipStream_t)stream);
}

int rdyhip_apply_phase(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *f_global, void *stream) {
  if (phase != RDYHIP_PHASE_ALL && phase != RDYHIP_PHASE_INTERIOR && phase != RDYHIP_PHASE_HALO) return fail(RDYHIP_ERR_USER, "bad phase %d", phase);
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  const int reset = (flags & RDYHIP_PHASE_RESET_DIAGNOSTICS) ? 1 : 0;
  if (reset) op->courant = RDyHipCourant{0.0, -1, -1};
  if (reset && phase == RDYHIP_PHASE_HALO && (op->use_tiled ? op->n_halo_tiles == 0 : op->n_halo == 0)) {
    int rc = rdyhip_reset_diagnostics(op, stream);  // nothing to launch in this phase: reset on its own
    if (rc) return rc;
  }
  return launch_rhs(op, phase, (flags & RDYHIP_PHASE_OVERWRITE) ? 1 : 0, reset, dt, u_local, f_global, (hipStream_t)stream,
                    (flags & RDYHIP_PHASE_GRADIENTS_READY) != 0);
}

int rdyhip_euler_step(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *u_local_out, double *f_global,
                      void *stream) {
  if (phase != RDYHIP_PHASE_ALL && phase != RDYHIP_PHASE_INTERIOR && phase != RDYHIP_PHASE_HALO) return fail(RDYHIP_ERR_USER, "bad phase %d", phase);
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->n_owned > 0 && (!u_local_out || u_local_out == u_local)) return fail(RDYHIP_ERR_USER, "rdyhip_euler_step needs a second state array (not in place)");
  const int reset = (flags & RDYHIP_PHASE_RESET_DIAGNOSTICS) ? 1 : 0;
  if (reset) op->courant = RDyHipCourant{0.0, -1, -1};
  if (reset && phase == RDYHIP_PHASE_HALO && (op->use_tiled ? op->n_halo_tiles == 0 : op->n_halo == 0)) {
    int rc = rdyhip_reset_diagnostics(op, stream);
    if (rc) return rc;
  }
  return launch_rhs(op, phase, 1, reset, dt, u_local, f_global, (hipStream_t)stream, (flags & RDYHIP_PHASE_GRADIENTS_READY) != 0, u_local_out);
}

int rdyhip_get_boundary_fluxes(RDyHipOperator op, int32_t boundary, int32_t accumulated, int32_t num_edges, double *fluxes) {
  int32_t off = 0, n = 0;
  int     rc  = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  if (!fluxes) return fail(RDYHIP_ERR_USER, "null output");
  const double *src = (accumulated ? op->d_baccum.p : op->d_bflux.p) + 3 * (size_t)off;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(fluxes, src, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

int rdyhip_reset_boundary_fluxes_accum(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(op->d_baccum.p, 0, std::max<size_t>(op->d_baccum.bytes(), sizeof(double))));
  return 0;
}

// The primitive variables leave the library: from now on every launch stores them (as every launch did before they became
// optional), and if evaluations have run without storing, the array is brought up to date first -- all owned rows, from the
// input state of the most recent of them, on the stream the caller ordered that evaluation on.
static int pv_hand_out(RDyHipOperator op) {
  op->pv_wanted = true;
  if (!op->pv_pending) return 0;
  op->pv_pending = false;  // whatever happens below: the next evaluation stores
  const double *u = op->pv_u;
  op->pv_u        = nullptr;
  if (op->n_owned == 0) return 0;
  // the remembered array is the caller's: launch nothing on a pointer the runtime does not know as memory of this device
  // (an array that was freed and allocated again, or overwritten since, cannot be told: see rdyhip_field_ptr in rdyhip.h)
  hipPointerAttribute_t at{};
  const hipError_t      e = u ? hipPointerGetAttributes(&at, u) : hipErrorInvalidValue;
  if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != op->device) {
    (void)hipGetLastError();
    return fail(RDYHIP_ERR_USER, "primitive variables: the state array of the last evaluation is gone (not device memory of device %d any more); "
                                 "the next evaluation will store them", op->device);
  }
  hipLaunchKernelGGL(primitive_variables_kernel, dim3((unsigned)((op->n_owned + 255) / 256)), dim3(256), 0, op->pv_stream, op->n_owned,
                     op->prefix ? nullptr : op->d_o2l.p, op->config.tiny_h, op->config.h_anuga_regular * op->config.h_anuga_regular, u, op->d_pv.p);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_field_ptr(RDyHipOperator op, RDyHipField field, double **device_ptr, int64_t *num_values) {
  int rc = field_ptr_internal(op, field, device_ptr, num_values);
  if (rc) return rc;
  if (field == RDYHIP_FIELD_PRIMITIVE_VARIABLES) return pv_hand_out(op);
  if (field == RDYHIP_FIELD_EXTERNAL_SOURCES) {
    // the caller may write the array in place at any time from now on: the water plane cannot be kept, for good
    op->src_escaped    = true;
    op->src_water_only = false;
    op->uniform.source.escape();
  }
  if (field == RDYHIP_FIELD_MANNINGS) op->uniform.mannings.escape();
  return 0;
}

int rdyhip_field_ptr_const(RDyHipOperator op, RDyHipField field, const double **device_ptr, int64_t *num_values) {
  double *p = nullptr;
  int     rc = field_ptr_internal(op, field, device_ptr ? &p : nullptr, num_values);
  if (rc) return rc;
  *device_ptr = p;
  if (field == RDYHIP_FIELD_PRIMITIVE_VARIABLES) return pv_hand_out(op);
  return 0;
}

int rdyhip_field_release(RDyHipOperator op, RDyHipField field) {
  if (field != RDYHIP_FIELD_PRIMITIVE_VARIABLES) return fail(RDYHIP_ERR_USER, "only the primitive variables can be released (field %d)", (int)field);
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  op->pv_wanted = false;  // the array stays as the last storing evaluation left it until somebody asks again
  return 0;
}

int rdyhip_primitive_variables_stored(RDyHipOperator op, int32_t *out) {
  if (!op || !out) return fail(RDYHIP_ERR_USER, "null argument");
  *out = op->pv_wanted ? 1 : 0;
  return 0;
}

int rdyhip_source_is_water_only(RDyHipOperator op, int32_t *out) {
  if (!op || !out) return fail(RDYHIP_ERR_USER, "null argument");
  *out = op->src_water_only ? 1 : 0;
  return 0;
}

static_assert(UNIFORM_SOURCE == RDYHIP_UNIFORM_SOURCE && UNIFORM_MANNINGS == RDYHIP_UNIFORM_MANNINGS && UNIFORM_FLAT_BED == RDYHIP_UNIFORM_FLAT_BED &&
                  (UNIFORM_SOURCE << 1) == STREAM_UNIFORM_SOURCE && (UNIFORM_MANNINGS << 1) == STREAM_UNIFORM_MANNINGS &&
                  (UNIFORM_FLAT_BED << 1) == STREAM_FLAT_BED,
              "rdyhip.h, uniform_fields.h and the kernels' stream flags name the same bits (launch_rhs shifts the mask by one)");
int rdyhip_uniform_fields(RDyHipOperator op, int32_t *mask) {
  if (!op || !mask) return fail(RDYHIP_ERR_USER, "null argument");
  *mask = op->uniform.mask(op->src_water_only);
  return 0;
}

int rdyhip_enable_flux_divergence(RDyHipOperator op, int32_t enable) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (enable && !op->d_fdiv.p) {
    int rc = op->d_fdiv.zeros((size_t)3 * op->n_owned);
    if (rc) return rc;
  }
  op->keep_fdiv = enable != 0;
  return 0;
}

int rdyhip_reset_diagnostics(RDyHipOperator op, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  hipLaunchKernelGGL(courant_reset_kernel, dim3(4), dim3(1024), 0, (hipStream_t)stream, (int)op->d_blk_max.n, op->d_blk_max.p, op->d_blk_pos.p);
  HIP_TRY(hipGetLastError());
  op->courant = RDyHipCourant{0.0, -1, -1};
  return 0;
}

// the device's (value, position in the reference's loop order) as the value and the global ids of its edge and cell
static RDyHipCourant courant_from_device(RDyHipOperator op, const DeviceCourant &dc) {
  RDyHipCourant out{dc.max_courant, -1, -1};
  if (dc.pos >= 0) {
    int32_t edge, cell;
    if (dc.pos < op->n_internal) {
      edge             = op->h_internal_edge[dc.pos];
      const int32_t l  = op->h_edge_cells[2 * (size_t)edge], r = op->h_edge_cells[2 * (size_t)edge + 1];
      cell             = (op->h_area[l] < op->h_area[r]) ? l : r;  // swe_petsc.c:294-295
    } else {
      const int32_t k = dc.pos - op->n_internal;
      edge            = op->h_bedge[k];
      cell            = op->h_edge_cells[2 * (size_t)edge];
    }
    out.global_edge_id = op->h_edge_gid.empty() ? edge : op->h_edge_gid[edge];
    out.global_cell_id = op->h_cell_gid.empty() ? cell : op->h_cell_gid[cell];
  }
  return out;
}

int rdyhip_update_diagnostics(RDyHipOperator op, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  // the RHS launches keep one running (max, first position) bucket per workgroup slot; they are merged only here
  hipLaunchKernelGGL(courant_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (int)op->d_blk_max.n, op->d_blk_max.p, op->d_blk_pos.p,
                     op->d_courant.p);
  HIP_TRY(hipGetLastError());
  DeviceCourant dc;
  HIP_TRY(hipMemcpyAsync(&dc, op->d_courant.p, sizeof(dc), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  op->courant = courant_from_device(op, dc);
  return 0;
}

int rdyhip_get_diagnostics(RDyHipOperator op, RDyHipCourant *courant) {
  if (!op || !courant) return fail(RDYHIP_ERR_USER, "null argument");
  *courant = op->courant;
  return 0;
}

int rdyhip_pack_cells(const double *u_local, const int32_t *cell_ids, int32_t n, double *buf, void *stream) {
  if (n < 0) return fail(RDYHIP_ERR_ARG_SIZ, "negative count");
  if (n == 0) return 0;
  if (!u_local || !cell_ids || !buf) return fail(RDYHIP_ERR_USER, "null argument");
  hipLaunchKernelGGL(pack_cells_kernel, dim3((unsigned)((3 * (int64_t)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, u_local, cell_ids, buf);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_unpack_cells(double *u_local, const int32_t *cell_ids, int32_t n, const double *buf, void *stream) {
  if (n < 0) return fail(RDYHIP_ERR_ARG_SIZ, "negative count");
  if (n == 0) return 0;
  if (!u_local || !cell_ids || !buf) return fail(RDYHIP_ERR_USER, "null argument");
  hipLaunchKernelGGL(unpack_cells_kernel, dim3((unsigned)((3 * (int64_t)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, u_local, cell_ids, buf);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_pack_rows(const double *src, int32_t ncomp, const int32_t *row_ids, int32_t n, double *buf, void *stream) {
  if (n < 0 || ncomp < 1) return fail(RDYHIP_ERR_ARG_SIZ, "bad count");
  if (n == 0) return 0;
  if (!src || !row_ids || !buf) return fail(RDYHIP_ERR_USER, "null argument");
  const int64_t tot = (int64_t)n * ncomp;
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, ncomp, src, row_ids, buf);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_unpack_rows(double *dst, int32_t ncomp, const int32_t *row_ids, int32_t n, const double *buf, void *stream) {
  if (n < 0 || ncomp < 1) return fail(RDYHIP_ERR_ARG_SIZ, "bad count");
  if (n == 0) return 0;
  if (!dst || !row_ids || !buf) return fail(RDYHIP_ERR_USER, "null argument");
  const int64_t tot = (int64_t)n * ncomp;
  hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, ncomp, dst, row_ids, buf);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_compute_gradients(RDyHipOperator op, int32_t phase, const double *u_local, void *stream) {
  return launch_gradients(op, phase, u_local, (hipStream_t)stream);
}

int rdyhip_axpy_owned(RDyHipOperator op, double dt, const double *f_global, double *u_local, void *stream) {
  if (!op || !f_global || !u_local) return fail(RDYHIP_ERR_USER, "null argument");
  if (op->n_owned == 0) return 0;
  const int64_t n3 = 3 * (int64_t)op->n_owned;
  hipLaunchKernelGGL(axpy_owned_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op->n_owned, op->prefix ? nullptr : op->d_o2l.p, dt,
                     f_global, u_local);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_copy_owned_rows(RDyHipOperator op, const double *u_global, double *u_local, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->n_owned == 0) return 0;
  if (!u_global || !u_local) return fail(RDYHIP_ERR_USER, "null argument");
  if (op->prefix) {  // the owned cells are the first rows of the local vector: one contiguous copy
    if (u_global != u_local)
      HIP_TRY(hipMemcpyAsync(u_local, u_global, sizeof(double) * 3 * (size_t)op->n_owned, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
  }
  if (u_global == u_local) return fail(RDYHIP_ERR_USER, "rdyhip_copy_owned_rows in place needs owned cells numbered first");
  const int64_t n3 = 3 * (int64_t)op->n_owned;
  hipLaunchKernelGGL(copy_owned_rows_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op->n_owned, op->d_o2l.p, u_global, u_local);
  HIP_TRY(hipGetLastError());
  return 0;
}

int32_t rdyhip_tiled_workgroups_per_cu(int32_t slots_per_cell, int32_t source_method, int32_t hydrostatic_reconstruction) {
  if ((slots_per_cell != 3 && slots_per_cell != 4) || (source_method != RDYHIP_SOURCE_SEMI_IMPLICIT && source_method != RDYHIP_SOURCE_IMPLICIT_XQ2018)) return 0;
  return tiled_blocks_per_cu(slots_per_cell, source_method == RDYHIP_SOURCE_IMPLICIT_XQ2018 ? 1 : 0, hydrostatic_reconstruction != 0);
}

int rdyhip_probe_layout(const RDyHipConfig *config, const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries,
                        RDyHipLayoutInfo *info) {
  if (!info) return fail(RDYHIP_ERR_USER, "null argument");
  HostLayout L;
  const int  rc = build_host_layout(config, mesh, num_boundaries, boundaries, L);
  if (!rc) fill_layout_info(L.counts, true, 0, 0, info);  // nothing is allocated on a device
  return rc;
}

int rdyhip_layout_info(RDyHipOperator op, RDyHipLayoutInfo *info) {
  if (!op || !info) return fail(RDYHIP_ERR_USER, "null argument");
  fill_layout_info(*op, op->use_tiled, op->muscl ? op->pgrid_muscl : op->pgrid, op->device_bytes, info);
  return 0;
}

}  // extern "C"

#include "halo_exchange.h"
#include "halo_plan.h"

// ---- classical Runge-Kutta step (rk_kernels.h) ------------------------------------------------------------------------------
namespace {

// the workspace of rdyhip_rk4_step, on its first call (hipMalloc: this one call may synchronise the device)
int rk4_workspace(RDyHipOperator op) {
  if (op->rk_ready) return 0;
  int rc = op->d_rk_y.alloc((size_t)3 * op->n_cells);
  for (auto &k : op->d_rk_k)
    if (!rc) rc = k.alloc((size_t)3 * op->n_owned);
  if (rc) {
    op->d_rk_y.release();
    for (auto &k : op->d_rk_k) k.release();
    return rc;
  }
  op->device_bytes += op->d_rk_y.bytes();
  for (auto &k : op->d_rk_k) op->device_bytes += k.bytes();
  op->rk_ready = true;
  return 0;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// y = u0 + c k on the owned rows; with `ghost_rows`, y's other rows = u0's
int launch_rk4_stage(RDyHipOperator op, double c, const double *k, const double *u0, double *y, bool ghost_rows, hipStream_t st) {
  const int64_t n_own = 3 * (int64_t)op->n_owned, n_cells3 = 3 * (int64_t)op->n_cells;
  if (!op->prefix) {
    if (ghost_rows && n_cells3 > 0) HIP_TRY(hipMemcpyAsync(y, u0, sizeof(double) * (size_t)n_cells3, hipMemcpyDeviceToDevice, st));
    if (n_own == 0) return 0;
    hipLaunchKernelGGL((rk4_stage_kernel<false>), dim3((unsigned)((n_own + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own, n_own,
                       op->d_o2l.p, c, k, u0, y);
  } else {
    const int64_t n_all = ghost_rows ? n_cells3 : n_own;
    if (n_all == 0) return 0;
    if (aligned16(k) && aligned16(u0) && aligned16(y)) {
      const int64_t pairs = (n_all + 1) / 2;
      hipLaunchKernelGGL((rk4_stage_kernel<true>), dim3((unsigned)((pairs + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own, n_all,
                         (const int32_t *)nullptr, c, k, u0, y);
    } else {
      hipLaunchKernelGGL((rk4_stage_kernel<false>), dim3((unsigned)((n_all + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own, n_all,
                         (const int32_t *)nullptr, c, k, u0, y);
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int launch_rk4_combine(RDyHipOperator op, double dt, double *u, hipStream_t st) {
  const int64_t n_own = 3 * (int64_t)op->n_owned;
  if (n_own == 0) return 0;
  const double  c1 = (1.0 / 6.0) * dt, c2 = (1.0 / 3.0) * dt, c3 = (1.0 / 3.0) * dt, c4 = (1.0 / 6.0) * dt;
  const double *k1 = op->d_rk_k[0].p, *k2 = op->d_rk_k[1].p, *k3 = op->d_rk_k[2].p, *k4 = op->d_rk_k[3].p;
  if (op->prefix && aligned16(u) && aligned16(k1) && aligned16(k2) && aligned16(k3) && aligned16(k4)) {
    const int64_t pairs = (n_own + 1) / 2;
    hipLaunchKernelGGL((rk4_combine_kernel<true>), dim3((unsigned)((pairs + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own,
                       (const int32_t *)nullptr, c1, c2, c3, c4, k1, k2, k3, k4, u);
  } else {
    hipLaunchKernelGGL((rk4_combine_kernel<false>), dim3((unsigned)((n_own + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own,
                       op->prefix ? (const int32_t *)nullptr : op->d_o2l.p, c1, c2, c3, c4, k1, k2, k3, k4, u);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int rdyhip_rk4_step(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->n_cells > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");   // (ghost rows alone are still copied and exchanged)
  if (halo && halo->op != op) return fail(RDYHIP_ERR_USER, "the halo belongs to another operator");
  hipStream_t st = (hipStream_t)stream;
  // the combine kernel writes the owned rows of u_local: a send buffer that mirrors them (rdyhip_halo_fuse_pack) is stale
  if (halo) halo_forget_packed_state(halo);
  if (op->fused_halo && op->fused_halo != halo) halo_forget_packed_state(op->fused_halo);
  int rc = rk4_workspace(op);
  if (rc) return rc;
  const bool exchange = halo && !halo->peers.empty();
  // every stage is OperatorRHSFunction with its ghost update and the FULL step's dt (TSGetTimeStep, src/rdysetup.c:1129)
  auto stage_rhs = [&](double *u, double *k) -> int {
    return exchange ? overlapped(op, halo, dt, u, k, nullptr, st) : rdyhip_rhs_function(op, dt, u, k, stream);
  };
  // the stage state's ghost rows: the stage's own exchange writes them where the halo receives every one of them; the
  // others keep u_local's values
  const bool ghost_rows = op->n_cells > op->n_owned && !(exchange && halo->recv_covers_ghosts);
  double    *y = op->d_rk_y.p;
  rc = stage_rhs(u_local, op->d_rk_k[0].p);
  const double a[3] = {0.5, 0.5, 1.0};
  for (int j = 1; j < 4 && !rc; ++j) {
    rc = launch_rk4_stage(op, a[j - 1] * dt, op->d_rk_k[j - 1].p, u_local, y, ghost_rows, st);
    if (!rc) rc = stage_rhs(y, op->d_rk_k[j].p);
  }
  if (!rc) rc = launch_rk4_combine(op, dt, u_local, st);
  return rc;
}

// ---- time-averaged output fields (output_kernels.h) ---------------------------------------------------------------------------
namespace {

constexpr int32_t OUT_VARS = RDYHIP_OUTPUT_SOLUTION | RDYHIP_OUTPUT_PRIMITIVE_VARIABLES | RDYHIP_OUTPUT_SOURCES;

// null operator, unknown bits, a variable without an accumulator: the argument errors the five calls share
int output_check(RDyHipOperator op, int32_t vars, bool single) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (vars & ~OUT_VARS) return fail(RDYHIP_ERR_USER, "unknown output variable bits 0x%x", (unsigned)(vars & ~OUT_VARS));
  if (single && vars != RDYHIP_OUTPUT_SOLUTION && vars != RDYHIP_OUTPUT_PRIMITIVE_VARIABLES && vars != RDYHIP_OUTPUT_SOURCES)
    return fail(RDYHIP_ERR_USER, "exactly one output variable is needed (got 0x%x)", (unsigned)vars);
  return 0;
}
int output_check_enabled(RDyHipOperator op, int32_t vars) {
  for (int i = 0; i < 3; ++i)
    if ((vars >> i & 1) && !op->d_out_acc[i].p)
      return fail(RDYHIP_ERR_USER, "output variable 0x%x is not enabled (rdyhip_output_mean_enable)", 1u << i);
  return 0;
}
int output_index(int32_t var) { return var == RDYHIP_OUTPUT_SOLUTION ? 0 : var == RDYHIP_OUTPUT_PRIMITIVE_VARIABLES ? 1 : 2; }

}  // namespace

extern "C" int rdyhip_output_mean_enable(RDyHipOperator op, int32_t vars) {
  int rc = output_check(op, vars, false);
  if (rc) return rc;
  for (int i = 0; i < 3; ++i) {
    DevBuf<double> &a = op->d_out_acc[i];
    if (!(vars >> i & 1) || a.p) continue;   // an existing accumulator keeps its content
    rc = a.zeros((size_t)3 * op->n_owned);
    if (rc) {
      a.release();
      return rc;
    }
    op->out_time[i] = 0.0;
    op->device_bytes += a.bytes();
  }
  return 0;
}

extern "C" int rdyhip_output_mean_accumulate(RDyHipOperator op, int32_t vars, double dt, const double *u_local, void *stream) {
  int rc = output_check(op, vars, false);
  if (!rc) rc = output_check_enabled(op, vars);
  if (rc) return rc;
  const bool sol = vars & RDYHIP_OUTPUT_SOLUTION, prim = vars & RDYHIP_OUTPUT_PRIMITIVE_VARIABLES, src = vars & RDYHIP_OUTPUT_SOURCES;
  if (sol && op->n_owned > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local (needed with RDYHIP_OUTPUT_SOLUTION)");
  if (op->n_owned > 0 && vars) {
    // The primitive variables of the most recent evaluation: the stored array while the evaluations store (or none has run
    // since the last store: the zeros of create included), else formed from that evaluation's state, which is the caller's
    // array -- checked as pv_hand_out checks it.  pv_wanted / pv_pending and the modes of the source are left as they are.
    // (After a pv_hand_out that failed on its own check, pv_wanted is on with d_pv not brought up to date: the stored rows are
    // then the last storing evaluation's until the next evaluation writes them -- rdyhip.h says so -- and are summed as such.)
    const double *u_prev = nullptr, *pv_stored = nullptr;
    if (prim) {
      if (op->pv_wanted || !op->pv_pending) {
        pv_stored = op->d_pv.p;
      } else {
        u_prev = op->pv_u;
        hipPointerAttribute_t at{};
        const hipError_t      e = u_prev ? hipPointerGetAttributes(&at, u_prev) : hipErrorInvalidValue;
        if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != op->device) {
          (void)hipGetLastError();
          return fail(RDYHIP_ERR_USER, "output means: the state array of the last evaluation is gone (not device memory of device %d any more)",
                      op->device);
        }
      }
    }
    const double *us = sol ? u_local : nullptr, *ext = src ? op->d_extsrc.p : nullptr;
    double       *acc_s = sol ? op->d_out_acc[0].p : nullptr, *acc_p = prim ? op->d_out_acc[1].p : nullptr, *acc_x = src ? op->d_out_acc[2].p : nullptr;
    const double  tiny_h = op->config.tiny_h, ha2 = op->config.h_anuga_regular * op->config.h_anuga_regular;
    hipLaunchKernelGGL(output_accumulate_kernel, dim3((unsigned)((op->n_owned + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, (hipStream_t)stream,
                       op->n_owned, op->prefix ? (const int32_t *)nullptr : op->d_o2l.p, dt, us, acc_s, u_prev, pv_stored, tiny_h, ha2, acc_p, ext, acc_x);
    HIP_TRY(hipGetLastError());
  }
  for (int i = 0; i < 3; ++i)
    if (vars >> i & 1) op->out_time[i] += dt;   // AccumulateOutputVar: accumulated_time += dt
  return 0;
}

extern "C" int rdyhip_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean, double *accumulated_time, void *stream) {
  int rc = output_check(op, var, true);
  if (!rc) rc = output_check_enabled(op, var);
  if (rc) return rc;
  const int i = output_index(var);
  if (op->n_owned > 0 && !d_mean) return fail(RDYHIP_ERR_USER, "null d_mean");
  // ComputeMean's PetscCheck (src/xdmf_output.c:213)
  if (!(op->out_time[i] > 0.0)) return fail(RDYHIP_ERR_USER, "output variable 0x%x: no time has been accumulated", (unsigned)var);
  if (accumulated_time) *accumulated_time = op->out_time[i];
  const int64_t n = 3 * (int64_t)op->n_owned;
  if (n == 0) return 0;
  const double  s   = 1.0 / op->out_time[i];
  const double *acc = op->d_out_acc[i].p;
  if (aligned16(acc) && aligned16(d_mean)) {
    const int64_t pairs = (n + 1) / 2;
    hipLaunchKernelGGL((output_mean_kernel<true>), dim3((unsigned)((pairs + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, (hipStream_t)stream, n, s,
                       acc, d_mean);
  } else {
    hipLaunchKernelGGL((output_mean_kernel<false>), dim3((unsigned)((n + OUT_BLOCK - 1) / OUT_BLOCK)), dim3(OUT_BLOCK), 0, (hipStream_t)stream, n, s, acc,
                       d_mean);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int rdyhip_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream) {
  int rc = output_check(op, vars, false);
  if (!rc) rc = output_check_enabled(op, vars);
  if (rc) return rc;
  for (int i = 0; i < 3; ++i) {
    if (!(vars >> i & 1)) continue;
    if (op->n_owned > 0) HIP_TRY(hipMemsetAsync(op->d_out_acc[i].p, 0, op->d_out_acc[i].bytes(), (hipStream_t)stream));
    op->out_time[i] = 0.0;
  }
  return 0;
}

extern "C" int rdyhip_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_time) {
  int rc = output_check(op, var, true);
  if (rc) return rc;
  if (!accumulated_time) return fail(RDYHIP_ERR_USER, "null accumulated_time");
  rc = output_check_enabled(op, var);
  if (rc) return rc;
  *accumulated_time = op->out_time[output_index(var)];
  return 0;
}

// ---- time series on the device (series_kernels.h, series_plan.h) ---------------------------------------------------------------
namespace {

// null operator, unknown kind: the argument errors every call shares; *s = the series
int series_check(RDyHipOperator op, int32_t kind, RDyHipOperator_s::Series **s) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (kind != RDYHIP_SERIES_OBSERVATIONS && kind != RDYHIP_SERIES_BOUNDARY_FLUXES)
    return fail(RDYHIP_ERR_USER, "unknown series kind %d (exactly one of RDYHIP_SERIES_OBSERVATIONS, RDYHIP_SERIES_BOUNDARY_FLUXES)", kind);
  *s = &op->series[kind == RDYHIP_SERIES_OBSERVATIONS ? 0 : 1];
  return 0;
}
int series_check_enabled(const RDyHipOperator_s::Series *s, int32_t kind) {
  if (!s->enabled) return fail(RDYHIP_ERR_USER, "series %d is not enabled (rdyhip_series_%s_enable)", kind,
                               kind == RDYHIP_SERIES_OBSERVATIONS ? "observations" : "boundary_fluxes");
  return 0;
}
// the log of `capacity` records of `entries` rows; on failure nothing is kept
int series_alloc_log(RDyHipOperator_s::Series *s, int32_t entries, int32_t capacity) {
  int rc = s->d_log.zeros((size_t)capacity * (size_t)entries * 3);
  if (rc) {
    s->d_log.release();
    return rc;
  }
  s->entries  = entries;
  s->capacity = capacity;
  s->times.clear();
  s->times.reserve((size_t)capacity);
  s->enabled = true;
  return 0;
}

}  // namespace

extern "C" int rdyhip_series_observations_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids, int32_t capacity) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (num_sites < 0 || capacity < 0) return fail(RDYHIP_ERR_USER, "negative number of sites (%d) or capacity (%d)", num_sites, capacity);
  if (num_sites > 0 && !owned_cell_ids) return fail(RDYHIP_ERR_USER, "null owned_cell_ids");
  RDyHipOperator_s::Series *s = &op->series[0];
  if (s->enabled) return fail(RDYHIP_ERR_USER, "the observation series is enabled already");
  for (int32_t i = 0; i < num_sites; ++i)
    if (owned_cell_ids[i] < 0 || owned_cell_ids[i] >= op->n_owned)
      return fail(RDYHIP_ERR_USER, "observation site %d: owned cell %d out of range [0, %d)", i, owned_cell_ids[i], op->n_owned);
  std::vector<int32_t> local(owned_cell_ids, owned_cell_ids + num_sites);
  if (!op->prefix && num_sites > 0) {   // owned -> local through the operator's own table
    std::vector<int32_t> o2l((size_t)op->n_owned);
    HIP_TRY(hipMemcpy(o2l.data(), op->d_o2l.p, sizeof(int32_t) * (size_t)op->n_owned, hipMemcpyDeviceToHost));
    for (auto &c : local) c = o2l[(size_t)c];
  }
  int rc = op->d_ser_sites.upload(local);
  if (!rc) rc = series_alloc_log(s, num_sites, capacity);
  if (rc) {
    op->d_ser_sites.release();
    return rc;
  }
  op->device_bytes += op->d_ser_sites.bytes() + s->d_log.bytes();
  return 0;
}

extern "C" int rdyhip_series_boundary_fluxes_enable(RDyHipOperator op, int32_t num_listed, const int32_t *boundaries, int32_t capacity) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (capacity < 0) return fail(RDYHIP_ERR_USER, "negative capacity (%d)", capacity);
  const int32_t        nb = (int32_t)op->h_boff.size() - 1;
  std::vector<uint8_t> mask;
  int                  rc = series_listed_mask(nb, num_listed, boundaries, mask);
  if (rc) return rc;
  RDyHipOperator_s::Series *s = &op->series[1];
  if (s->enabled) return fail(RDYHIP_ERR_USER, "the boundary-flux series is enabled already");
  std::vector<uint8_t> left_owned((size_t)op->K, 1);
  for (int32_t k : op->h_bghost) left_owned[(size_t)k] = 0;
  SeriesPlan P;
  series_plan_rows(nb, op->h_boff.data(), op->h_bedge.data(), left_owned.data(), mask, P);
  rc = op->d_ser_slot.upload(P.slot);
  if (!rc) rc = op->d_ser_len.upload(op->h_blen);
  if (!rc) rc = series_alloc_log(s, P.E, capacity);
  if (rc) {
    op->d_ser_slot.release();
    op->d_ser_len.release();
    return rc;
  }
  op->h_ser_edge = std::move(P.edge);
  op->h_ser_bnd  = std::move(P.boundary);
  op->ser_btime  = 0.0;
  op->device_bytes += op->d_ser_slot.bytes() + op->d_ser_len.bytes() + s->d_log.bytes();
  return 0;
}

extern "C" int rdyhip_series_boundary_edges(RDyHipOperator op, int32_t *num_edges, const int32_t **local_edge_ids, const int32_t **boundary_of_edge) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  int rc = series_check_enabled(&op->series[1], RDYHIP_SERIES_BOUNDARY_FLUXES);
  if (rc) return rc;
  if (num_edges) *num_edges = op->series[1].entries;
  if (local_edge_ids) *local_edge_ids = op->h_ser_edge.data();
  if (boundary_of_edge) *boundary_of_edge = op->h_ser_bnd.data();
  return 0;
}

extern "C" int rdyhip_series_plan_boundary_edges(const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries, int32_t num_listed,
                                                 const int32_t *listed, int32_t *num_edges, int32_t *local_edge_ids, int32_t *boundary_of_edge) {
  if (!num_edges) return fail(RDYHIP_ERR_USER, "null num_edges");
  SeriesPlan P;
  int        rc = series_plan_from_mesh(mesh, num_boundaries, boundaries, num_listed, listed, P);
  if (rc) return rc;
  *num_edges = P.E;
  if (local_edge_ids) std::copy(P.edge.begin(), P.edge.end(), local_edge_ids);
  if (boundary_of_edge) std::copy(P.boundary.begin(), P.boundary.end(), boundary_of_edge);
  return 0;
}

extern "C" int rdyhip_series_boundary_fluxes_add_time(RDyHipOperator op, double dt) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  int rc = series_check_enabled(&op->series[1], RDYHIP_SERIES_BOUNDARY_FLUXES);
  if (rc) return rc;
  op->ser_btime += dt;   // AccumulateBoundaryFluxes: accumulated_time += dt
  return 0;
}

extern "C" int rdyhip_series_record(RDyHipOperator op, int32_t kind, double time, const double *u_local, void *stream) {
  RDyHipOperator_s::Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  const bool obs = kind == RDYHIP_SERIES_OBSERVATIONS;
  if (obs && s->entries > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local (needed with RDYHIP_SERIES_OBSERVATIONS)");
  if ((int64_t)s->times.size() >= (int64_t)s->capacity)
    return fail(RDYHIP_ERR_USER, "series %d: the log is full (%d records); read it and call rdyhip_series_clear", kind, s->capacity);
  const int64_t r = (int64_t)s->times.size();
  if (s->entries > 0) {
    if (obs) {
      hipLaunchKernelGGL(series_observe_kernel, dim3((unsigned)((s->entries + SERIES_BLOCK - 1) / SERIES_BLOCK)), dim3(SERIES_BLOCK), 0, (hipStream_t)stream,
                         s->entries, op->d_ser_sites.p, u_local, r, s->d_log.p);
    } else {
      // WriteBoundaryFluxes (src/time_series.c:311-313): no accumulated time divides by 1
      const double T = op->ser_btime == 0.0 ? 1.0 : op->ser_btime;
      hipLaunchKernelGGL(series_boundary_record_kernel, dim3((unsigned)((op->K + SERIES_BLOCK - 1) / SERIES_BLOCK)), dim3(SERIES_BLOCK), 0, (hipStream_t)stream,
                         op->K, op->d_ser_slot.p, op->d_ser_len.p, T, r, (int64_t)s->entries, op->d_baccum.p, s->d_log.p);
    }
    HIP_TRY(hipGetLastError());
  }
  s->times.push_back(time);
  if (!obs) op->ser_btime = 0.0;   // ResetAccumulatedBoundaryFluxes
  return 0;
}

extern "C" int rdyhip_series_info(RDyHipOperator op, int32_t kind, int32_t *entries, int32_t *count, int32_t *capacity, double *accumulated_time) {
  RDyHipOperator_s::Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  if (entries) *entries = s->entries;
  if (count) *count = (int32_t)s->times.size();
  if (capacity) *capacity = s->capacity;
  if (accumulated_time) *accumulated_time = kind == RDYHIP_SERIES_BOUNDARY_FLUXES ? op->ser_btime : 0.0;
  return 0;
}

extern "C" int rdyhip_series_read(RDyHipOperator op, int32_t kind, int32_t first, int32_t count, double *times, double *values, void *stream) {
  RDyHipOperator_s::Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  if (first < 0 || count < 0 || (int64_t)first + count > (int64_t)s->times.size())
    return fail(RDYHIP_ERR_USER, "series %d: records [%d, %d + %d) are not in the log (%d records)", kind, first, first, count, (int)s->times.size());
  const size_t row = (size_t)s->entries * 3;
  if (count > 0 && (!times || (row > 0 && !values))) return fail(RDYHIP_ERR_USER, "null times / values");
  if (count == 0) return 0;
  std::copy(s->times.begin() + first, s->times.begin() + first + count, times);
  if (row > 0)
    HIP_TRY(hipMemcpyAsync(values, s->d_log.p + (size_t)first * row, sizeof(double) * (size_t)count * row, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

extern "C" int rdyhip_series_device_log(RDyHipOperator op, int32_t kind, const double **d_log) {
  RDyHipOperator_s::Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (rc) return rc;
  if (!d_log) return fail(RDYHIP_ERR_USER, "null d_log");
  rc = series_check_enabled(s, kind);
  if (rc) return rc;
  *d_log = s->d_log.p;
  return 0;
}

extern "C" int rdyhip_series_clear(RDyHipOperator op, int32_t kind) {
  RDyHipOperator_s::Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  s->times.clear();
  return 0;
}

// ---- state read-out: owned-cell getters and error sums (readout_kernels.h) ----------------------------------------------------
namespace {

constexpr int32_t READ_COMPS = RDYHIP_COMPONENT_H | RDYHIP_COMPONENT_HU | RDYHIP_COMPONENT_HV;

int popcount3(int32_t comps) { return (comps & 1) + (comps >> 1 & 1) + (comps >> 2 & 1); }
bool one_component(int32_t comp) { return comp == RDYHIP_COMPONENT_H || comp == RDYHIP_COMPONENT_HU || comp == RDYHIP_COMPONENT_HV; }

int launch_state_planes(RDyHipOperator op, int32_t comps, const double *u, double *planes, hipStream_t st) {
  hipLaunchKernelGGL(state_planes_kernel, dim3((unsigned)((op->n_owned + READ_BLOCK - 1) / READ_BLOCK)), dim3(READ_BLOCK), 0, st, op->n_owned,
                     op->prefix ? (const int32_t *)nullptr : op->d_o2l.p, (int)comps, (const uint64_t *)u, (uint64_t *)planes);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the copy stream (shared with the setters' staging ring), the two events, and room for `k` planes on the device and in pinned
// memory: grows only; a call that allocates may synchronise, and waits first for a copy that still reads the old buffers
int read_reserve(RDyHipOperator op, int k) {
  Readout &r = op->readout;
  if (!op->stage.copy) HIP_TRY(hipStreamCreateWithFlags(&op->stage.copy, hipStreamNonBlocking));
  if (!r.launched) HIP_TRY(hipEventCreateWithFlags(&r.launched, hipEventDisableTiming));
  if (!r.done) HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  const size_t need = (size_t)k * (size_t)op->n_owned;
  if (r.d_planes.p && r.d_planes.n >= need && r.h_cap >= need) return 0;
  if (r.state == Readout::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.done));
  r.state = Readout::NONE;   // whatever had been read lived in the old buffers
  op->device_bytes -= (int64_t)r.d_planes.bytes();
  int rc = r.d_planes.alloc(need);
  if (rc) return rc;
  op->device_bytes += (int64_t)r.d_planes.bytes();
  if (r.h_planes) HIP_TRY(hipHostFree(r.h_planes));
  r.h_planes = nullptr;
  r.h_cap    = 0;
  HIP_TRY(hipHostMalloc((void **)&r.h_planes, sizeof(double) * need, hipHostMallocDefault));
  r.h_cap = need;
  return 0;
}

// the arguments of _get and _ptr; *plane = the index of `comp` among the planes of the last begin
int read_check_landed(RDyHipOperator op, int32_t comp, int *plane) {
  const Readout &r = op->readout;
  if (r.state != Readout::LANDED)
    return fail(RDYHIP_ERR_USER, r.state == Readout::NONE ? "no state read has been begun (rdyhip_state_read_begin)"
                                                          : "the state read has not been waited for (rdyhip_state_read_wait)");
  if (!(r.comps & comp)) return fail(RDYHIP_ERR_USER, "component 0x%x was not asked for by the last rdyhip_state_read_begin (0x%x)", (unsigned)comp, (unsigned)r.comps);
  *plane = popcount3(r.comps & (comp - 1));
  return 0;
}

// areas by owned cell, the partial records and the pinned result of the error sums, on the first call (may synchronise)
int sums_reserve(RDyHipOperator op) {
  Readout &r = op->readout;
  if (r.d_area.p) return 0;
  const size_t no = (size_t)op->n_owned;
  std::vector<double> area(no);
  if (op->prefix) {
    std::copy(op->h_area.begin(), op->h_area.begin() + no, area.begin());
  } else {
    std::vector<int32_t> o2l(no);
    HIP_TRY(hipMemcpy(o2l.data(), op->d_o2l.p, sizeof(int32_t) * no, hipMemcpyDeviceToHost));
    for (size_t o = 0; o < no; ++o) area[o] = op->h_area[(size_t)o2l[o]];
  }
  const int wg = (int)std::min<int64_t>(((int64_t)op->n_owned + ERR_BLOCK - 1) / ERR_BLOCK, ERR_MAX_WG);
  if (!r.sums_done) HIP_TRY(hipEventCreateWithFlags(&r.sums_done, hipEventDisableTiming));
  if (!r.h_sums) HIP_TRY(hipHostMalloc((void **)&r.h_sums, sizeof(double) * ERR_VALUES, hipHostMallocDefault));
  int rc = r.d_records.alloc((size_t)(wg + 1) * ERR_VALUES);
  if (!rc) rc = r.d_area.upload(area);
  if (rc) {
    r.d_records.release();
    r.d_area.release();
    return rc;
  }
  r.err_wg = wg;
  op->device_bytes += (int64_t)(r.d_area.bytes() + r.d_records.bytes());
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
  Readout &r = op->readout;
  if (op->n_owned == 0) {   // nothing is launched or copied: the read has landed as soon as it is waited for
    r.comps = comps;
    r.state = Readout::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  hipStream_t st = (hipStream_t)stream;
  const int   k  = popcount3(comps);
  int rc = read_reserve(op, k);
  if (rc) return rc;
  // an earlier read that has not landed is given up; its copy may still be reading the device planes, so this launch waits for it
  if (r.state == Readout::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.done, 0));
  r.state = Readout::NONE;
  rc = launch_state_planes(op, comps, u_local, r.d_planes.p, st);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(r.launched, st));
  HIP_TRY(hipStreamWaitEvent(op->stage.copy, r.launched, 0));
  HIP_TRY(hipMemcpyAsync(r.h_planes, r.d_planes.p, sizeof(double) * (size_t)k * (size_t)op->n_owned, hipMemcpyDeviceToHost, op->stage.copy));
  HIP_TRY(hipEventRecord(r.done, op->stage.copy));
  r.comps = comps;
  r.state = Readout::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_state_read_ready(RDyHipOperator op, int32_t *ready) {
  if (!op || !ready) return fail(RDYHIP_ERR_USER, "null argument");
  const Readout &r = op->readout;
  if (r.state == Readout::NONE) return fail(RDYHIP_ERR_USER, "no state read has been begun (rdyhip_state_read_begin)");
  *ready = 1;
  if (r.state == Readout::IN_FLIGHT && op->n_owned > 0) {
    const hipError_t e = hipEventQuery(r.done);
    if (e == hipErrorNotReady) {
      (void)hipGetLastError();
      *ready = 0;
    } else {
      HIP_TRY(e);
    }
  }
  return 0;
}

extern "C" int rdyhip_state_read_wait(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  Readout &r = op->readout;
  if (r.state == Readout::NONE) return fail(RDYHIP_ERR_USER, "no state read has been begun (rdyhip_state_read_begin)");
  if (r.state == Readout::IN_FLIGHT && op->n_owned > 0) HIP_TRY(hipEventSynchronize(r.done));
  r.state = Readout::LANDED;
  return 0;
}

extern "C" int rdyhip_state_read_get(RDyHipOperator op, int32_t comp, int32_t size, double *values) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (!one_component(comp)) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comp);
  // CheckNumOwnedCells (src/rdydata.c:54-58)
  if (size != op->n_owned) return fail(RDYHIP_ERR_ARG_SIZ, "The size of array (%d) is not equal to the number of owned cells (%d)", size, op->n_owned);
  if (size > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  int plane = 0;
  int rc = read_check_landed(op, comp, &plane);
  if (rc) return rc;
  if (size > 0) memcpy(values, op->readout.h_planes + (size_t)plane * (size_t)op->n_owned, sizeof(double) * (size_t)size);
  return 0;
}

extern "C" int rdyhip_state_read_ptr(RDyHipOperator op, int32_t comp, const double **pinned_values) {
  if (!op || !pinned_values) return fail(RDYHIP_ERR_USER, "null argument");
  if (!one_component(comp)) return fail(RDYHIP_ERR_USER, "exactly one component is needed (got 0x%x)", (unsigned)comp);
  int plane = 0;
  int rc = read_check_landed(op, comp, &plane);
  if (rc) return rc;
  *pinned_values = op->n_owned > 0 ? op->readout.h_planes + (size_t)plane * (size_t)op->n_owned : nullptr;
  return 0;
}

extern "C" int rdyhip_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  Readout &r = op->readout;
  if (op->n_owned == 0) {   // all zeros, nothing launched
    r.sums_state = Readout::IN_FLIGHT;
    return 0;
  }
  if (!u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  int rc = sums_reserve(op);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the records and the pinned result are shared by all calls: this one is ordered behind an earlier one that is still running
  if (r.sums_state == Readout::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.sums_done, 0));
  double *result = r.d_records.p + (size_t)r.err_wg * ERR_VALUES;
  hipLaunchKernelGGL(error_partial_kernel, dim3(r.err_wg), dim3(ERR_BLOCK), 0, st, op->n_owned, op->prefix ? (const int32_t *)nullptr : op->d_o2l.p,
                     u_local, d_exact, r.d_area.p, r.d_records.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(error_finalize_kernel, dim3(1), dim3(ERR_BLOCK), 0, st, r.err_wg, r.d_records.p, result);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(r.h_sums, result, sizeof(double) * ERR_VALUES, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(r.sums_done, st));
  r.sums_state = Readout::IN_FLIGHT;
  return 0;
}

extern "C" int rdyhip_error_sums_get(RDyHipOperator op, RDyHipErrorSums *out) {
  if (!op || !out) return fail(RDYHIP_ERR_USER, "null argument");
  Readout &r = op->readout;
  if (r.sums_state == Readout::NONE) return fail(RDYHIP_ERR_USER, "no error sums have been asked for (rdyhip_error_sums)");
  static_assert(sizeof(RDyHipErrorSums) == sizeof(double) * ERR_VALUES, "RDyHipErrorSums is the ten doubles of a record");
  if (op->n_owned == 0) {
    memset(out, 0, sizeof(*out));
  } else {
    if (r.sums_state == Readout::IN_FLIGHT) HIP_TRY(hipEventSynchronize(r.sums_done));
    memcpy(out, r.h_sums, sizeof(*out));
  }
  r.sums_state = Readout::LANDED;
  return 0;
}

// ---- shallow water with advected tracers (tracer_kernels.h) -------------------------------------------------------------------
namespace {

using TracerKernelFn = void (*)(const KernelArgs, const TracerArgs, const double, const double *);

// The instantiation of the tracer kernel for (slots per cell, number of tracers, upwind tracer flux): 2 x 7 x 2 = 28
template <int S, bool UPWIND>
TracerKernelFn tracer_kernel_nt(int nt) {
  switch (nt) {
    case 1: return tracer_rhs_kernel<S, 1, UPWIND>;
    case 2: return tracer_rhs_kernel<S, 2, UPWIND>;
    case 3: return tracer_rhs_kernel<S, 3, UPWIND>;
    case 4: return tracer_rhs_kernel<S, 4, UPWIND>;
    case 5: return tracer_rhs_kernel<S, 5, UPWIND>;
    case 6: return tracer_rhs_kernel<S, 6, UPWIND>;
    default: return tracer_rhs_kernel<S, 7, UPWIND>;
  }
}
TracerKernelFn tracer_kernel_fn(int S, int nt, bool upwind) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(upwind, [&](auto up) -> TracerKernelFn {
    return tracer_kernel_nt<quad ? 4 : 3, up>(nt);
  }); });
}

// null operator, tracers not enabled: what every call after rdyhip_tracers_enable starts with
int tracers_check(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->n_tracers == 0) return fail(RDYHIP_ERR_USER, "tracers are not enabled (rdyhip_tracers_enable)");
  return 0;
}

// One tracer evaluation: OperatorRHSFunction's zeroing of F, diagnostics reset and apply in one launch; with u_out the
// forward-Euler update rides on the stores (f may then be NULL)
int launch_tracers(RDyHipOperator op, double dt, const double *u, double *f, double *u_out, hipStream_t st) {
  if (op->n_owned == 0) return 0;   // a rank may own nothing: nothing to launch
  op->courant = RDyHipCourant{0.0, -1, -1};
  KernelArgs a{};
  a.n_owned    = op->n_owned;
  a.n_work     = op->n_owned;
  a.stride     = op->stride;
  a.o2l        = op->prefix ? nullptr : op->d_o2l.p;
  a.cold       = op->d_cold.p;
  a.coef       = op->d_coef.p;
  a.dzdx       = op->d_dzdx.p;
  a.dzdy       = op->d_dzdy.p;
  a.mannings   = op->d_mannings.p;
  a.extsrc     = op->d_extsrc.p;   // the canonical [owned][3] array, whatever the water-only mode of the SWE kernels says
  a.src_mom    = 1;
  a.n_buckets  = (int32_t)op->d_blk_max.n;
  a.bucket_off = 0;
  a.reset_diag = 1;
  a.tiny_h     = op->config.tiny_h;
  a.h_anuga_sq = op->config.h_anuga_regular * op->config.h_anuga_regular;
  a.xq_thresh  = op->config.xq2018_threshold;
  a.overwrite  = 1;
  a.phase      = RDYHIP_PHASE_ALL;
  a.xcd_chunks = op->xcd_chunks;
  TracerArgs t{};
  t.bvalues = op->d_tr_bvalues.p;
  t.bflux   = op->d_tr_bflux.p;
  t.src     = op->d_tr_src.p;
  t.pv      = op->tr_pv_wanted ? op->d_tr_pv.p : nullptr;   // read here, when the launch is enqueued
  t.f       = f;
  t.u_out   = u_out;
  TracerKernelFn kfn = tracer_kernel_fn(op->S, op->n_tracers, op->tracer_riemann == RDYHIP_TRACER_RIEMANN_UPWIND_ROE);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(op->grid), dim3(BLOCK), 0, st, a, t, dt, u);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int rdyhip_tracers_enable(RDyHipOperator op, int32_t num_tracers, int32_t riemann) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->n_tracers != 0) return fail(RDYHIP_ERR_USER, "tracers are already enabled (%d)", op->n_tracers);
  if (num_tracers < 1 || num_tracers > RDYHIP_MAX_TRACERS)
    return fail(RDYHIP_ERR_USER, "num_tracers (%d) must be in 1..%d", num_tracers, RDYHIP_MAX_TRACERS);
  if (riemann != RDYHIP_TRACER_RIEMANN_ROE && riemann != RDYHIP_TRACER_RIEMANN_UPWIND_ROE)
    return fail(RDYHIP_ERR_USER, "unknown tracer Riemann solver %d", riemann);
  if (op->muscl || op->config.second_order) return fail(RDYHIP_ERR_USER, "tracers are first order only (the operator was created with second_order)");
  if (op->hr || op->config.well_balancing != RDYHIP_WELL_BALANCING_NONE)
    return fail(RDYHIP_ERR_USER, "tracers with well balancing are not supported (well_balancing = %d)", op->config.well_balancing);
  if (op->config.source_method != RDYHIP_SOURCE_SEMI_IMPLICIT)
    return fail(RDYHIP_ERR_USER, "tracers have the semi-implicit source only (source_method = %d)", op->config.source_method);
  for (size_t k = 0; k < op->h_btype.size(); ++k)
    if (op->h_btype[k] == RDYHIP_CONDITION_CRITICAL_OUTFLOW)
      return fail(RDYHIP_ERR_USER, "CONDITION_CRITICAL_OUTFLOW not supported for tracers");   // tracer_petsc.c:472-474
    else if (op->h_btype[k] != RDYHIP_CONDITION_DIRICHLET && op->h_btype[k] != RDYHIP_CONDITION_REFLECTING)
      return fail(RDYHIP_ERR_USER, "Invalid boundary condition %d encountered for tracers", op->h_btype[k]);
  const size_t N = 3 + (size_t)num_tracers, K = (size_t)op->K, no = (size_t)op->n_owned;
  int rc = op->d_tr_bvalues.zeros(N * K);
  if (!rc) rc = op->d_tr_bflux.zeros(N * K);
  if (!rc) rc = op->d_tr_src.zeros((size_t)num_tracers * no);
  if (rc) {
    op->d_tr_bvalues.release();
    op->d_tr_bflux.release();
    op->d_tr_src.release();
    return rc;
  }
  op->device_bytes += op->d_tr_bvalues.bytes() + op->d_tr_bflux.bytes() + op->d_tr_src.bytes();
  op->n_tracers      = num_tracers;
  op->tracer_riemann = riemann;
  return 0;
}

extern "C" int rdyhip_tracers_info(RDyHipOperator op, int32_t *num_tracers, int32_t *riemann) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (num_tracers) *num_tracers = op->n_tracers;
  if (riemann) *riemann = op->tracer_riemann;
  return 0;
}

extern "C" int rdyhip_tracers_set_boundary_values(RDyHipOperator op, int32_t boundary, int32_t num_edges, const double *values) {
  int rc = tracers_check(op);
  if (rc) return rc;
  int32_t off = 0, n = 0;
  rc = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  if (!values) return fail(RDYHIP_ERR_USER, "null values");
  const size_t N = 3 + (size_t)op->n_tracers;
  HIP_TRY(hipDeviceSynchronize());   // an evaluation in flight on a non-blocking stream may still read the values this call replaces
  HIP_TRY(hipMemcpy(op->d_tr_bvalues.p + N * (size_t)off, values, sizeof(double) * N * (size_t)n, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int rdyhip_tracers_set_source(RDyHipOperator op, int32_t tracer, int32_t n, const int32_t *owned_cell_ids, const double *values) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (tracer < 0 || tracer >= op->n_tracers) return fail(RDYHIP_ERR_USER, "tracer index %d out of range (%d tracers)", tracer, op->n_tracers);
  return scatter_component(op, op->d_tr_src.p, op->n_tracers, tracer, n, owned_cell_ids, values);
}

extern "C" int rdyhip_tracers_rhs_function(RDyHipOperator op, double dt, const double *u_local, double *f_global, void *stream) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (op->n_owned > 0 && (!u_local || !f_global)) return fail(RDYHIP_ERR_USER, "null u_local / f_global");
  return launch_tracers(op, dt, u_local, f_global, nullptr, (hipStream_t)stream);
}

extern "C" int rdyhip_tracers_euler_step(RDyHipOperator op, double dt, const double *u_local, double *u_local_out, double *f_global, void *stream) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (op->n_owned > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  if (op->n_owned > 0 && (!u_local_out || u_local_out == u_local))
    return fail(RDYHIP_ERR_USER, "rdyhip_tracers_euler_step needs a second state array (not in place)");
  return launch_tracers(op, dt, u_local, f_global, u_local_out, (hipStream_t)stream);
}

extern "C" int rdyhip_tracers_primitive_variables(RDyHipOperator op, const double **device_ptr, int64_t *num_values) {
  int rc = tracers_check(op);
  if (rc) return rc;
  if (!device_ptr) return fail(RDYHIP_ERR_USER, "null argument");
  const size_t n = (3 + (size_t)op->n_tracers) * (size_t)op->n_owned;
  if (!op->d_tr_pv.p) {
    rc = op->d_tr_pv.zeros(n);
    if (rc) {
      op->d_tr_pv.release();
      return rc;
    }
    op->device_bytes += op->d_tr_pv.bytes();
  }
  op->tr_pv_wanted = true;
  *device_ptr = op->d_tr_pv.p;
  if (num_values) *num_values = (int64_t)n;
  return 0;
}

extern "C" int rdyhip_tracers_get_boundary_fluxes(RDyHipOperator op, int32_t boundary, int32_t num_edges, double *fluxes) {
  int rc = tracers_check(op);
  if (rc) return rc;
  int32_t off = 0, n = 0;
  rc = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  if (!fluxes) return fail(RDYHIP_ERR_USER, "null output");
  const size_t N = 3 + (size_t)op->n_tracers;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(fluxes, op->d_tr_bflux.p + N * (size_t)off, sizeof(double) * N * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// ---- ensembles: B members on one mesh, one launch per evaluation (ensemble_kernels.h) --------------------------------------------
namespace {

using EnsembleKernelFn = void (*)(const KernelArgs, const EnsembleArgs, const double *);

// The instantiation of the ensemble kernel for (slots per cell, source method, the fused Euler update): 2 x 2 x 2 = 8
EnsembleKernelFn ensemble_kernel_fn(int S, int src, bool euler) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(src != 0, [&](auto xq) { return with_flag(euler, [&](auto eu) -> EnsembleKernelFn {
    return ensemble_rhs_kernel<quad ? 4 : 3, xq ? 1 : 0, eu>;
  }); }); });
}

// null operator, ensemble not enabled: what every call after rdyhip_ensemble_enable starts with; then the member index
int ensemble_check(RDyHipOperator op) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->ens_members == 0) return fail(RDYHIP_ERR_USER, "the ensemble is not enabled (rdyhip_ensemble_enable)");
  return 0;
}
int ensemble_check_member(RDyHipOperator op, int32_t member) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (member < 0 || member >= op->ens_members) return fail(RDYHIP_ERR_USER, "member index %d out of range (%d members)", member, op->ens_members);
  return 0;
}

// One evaluation of all members: per member OperatorRHSFunction's zeroing of F, diagnostics reset and apply; with u_out the
// forward-Euler update rides on the stores (f may then be NULL)
int launch_ensemble(RDyHipOperator op, const double *dts, const double *u, double *f, double *u_out, hipStream_t st) {
  for (auto &c : op->ens_courant) c = RDyHipCourant{0.0, -1, -1};
  if (op->n_owned == 0) return 0;   // a rank may own nothing: nothing to launch
  KernelArgs a{};
  a.n_owned    = op->n_owned;
  a.n_work     = op->n_owned;
  a.stride     = op->stride;
  a.o2l        = op->prefix ? nullptr : op->d_o2l.p;
  a.cold       = op->d_cold.p;
  a.coef       = op->d_coef.p;
  a.dzdx       = op->d_dzdx.p;
  a.dzdy       = op->d_dzdy.p;
  a.tiny_h     = op->config.tiny_h;
  a.h_anuga_sq = op->config.h_anuga_regular * op->config.h_anuga_regular;
  a.xq_thresh  = op->config.xq2018_threshold;
  a.overwrite  = 1;
  a.phase      = RDYHIP_PHASE_ALL;
  a.xcd_chunks = op->xcd_chunks;
  EnsembleArgs t{};
  t.mannings  = op->d_ens_mannings.p;
  t.extsrc    = op->d_ens_extsrc.p;
  t.bvalues   = op->d_ens_bvalues.p;
  t.bflux     = op->d_ens_bflux.p;
  t.blk_max   = op->d_ens_blk_max.p;
  t.blk_pos   = op->d_ens_blk_pos.p;
  t.f         = f;
  t.u_out     = u_out;
  t.u_stride  = 3 * (int64_t)op->n_cells;
  t.k_stride  = 3 * (int64_t)op->K;
  t.n_members = op->ens_members;
  t.per_group = op->ens_per_group;
  t.n_buckets = ENSEMBLE_WAVES * op->grid;
  for (int m = 0; m < op->ens_members; ++m) t.dts[m] = dts[m];
  EnsembleKernelFn kfn = ensemble_kernel_fn(op->S, op->config.source_method, u_out != nullptr);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(op->grid, op->ens_groups), dim3(BLOCK), 0, st, a, t, u);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int rdyhip_ensemble_enable(RDyHipOperator op, int32_t num_members) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->ens_members != 0) return fail(RDYHIP_ERR_USER, "the ensemble is already enabled (%d members)", op->ens_members);
  if (num_members < 1 || num_members > RDYHIP_MAX_ENSEMBLE_MEMBERS)
    return fail(RDYHIP_ERR_USER, "num_members (%d) must be in 1..%d", num_members, RDYHIP_MAX_ENSEMBLE_MEMBERS);
  if (op->muscl || op->config.second_order) return fail(RDYHIP_ERR_USER, "ensembles are first order only (the operator was created with second_order)");
  if (op->hr || op->config.well_balancing != RDYHIP_WELL_BALANCING_NONE)
    return fail(RDYHIP_ERR_USER, "ensembles with well balancing are not supported (well_balancing = %d)", op->config.well_balancing);
  const size_t B = (size_t)num_members, K = (size_t)op->K, no = (size_t)op->n_owned, W = (size_t)ENSEMBLE_WAVES * (size_t)op->grid;
  DevBuf<double> *bufs[] = {&op->d_ens_mannings, &op->d_ens_extsrc, &op->d_ens_bvalues, &op->d_ens_bflux, &op->d_ens_blk_max};
  int rc = op->d_ens_mannings.alloc(B * no);
  if (!rc) rc = op->d_ens_extsrc.alloc(B * 3 * no);
  if (!rc) rc = op->d_ens_bvalues.alloc(B * 3 * K);
  if (!rc) rc = op->d_ens_bflux.zeros(B * 3 * K);
  if (!rc) rc = op->d_ens_blk_max.zeros(B * W);
  if (!rc) rc = op->d_ens_blk_pos.zeros(B * W);
  if (!rc) rc = op->d_ens_courant.zeros(B);
  auto undo = [&](int code) {
    for (auto *b : bufs) b->release();
    op->d_ens_blk_pos.release();
    op->d_ens_courant.release();
    return code;
  };
  if (rc) return undo(rc);
  // every member starts with the operator's own Manning's n, source and boundary values (an evaluation in flight may not
  // write them, but a stream-ordered setter may: wait for it)
  hipError_t e = hipDeviceSynchronize();
  for (size_t m = 0; m < B && e == hipSuccess; ++m) {
    if (no) e = hipMemcpy(op->d_ens_mannings.p + m * no, op->d_mannings.p, sizeof(double) * no, hipMemcpyDeviceToDevice);
    if (no && e == hipSuccess) e = hipMemcpy(op->d_ens_extsrc.p + m * 3 * no, op->d_extsrc.p, sizeof(double) * 3 * no, hipMemcpyDeviceToDevice);
    if (K && e == hipSuccess) e = hipMemcpy(op->d_ens_bvalues.p + m * 3 * K, op->d_bvalues.p, sizeof(double) * 3 * K, hipMemcpyDeviceToDevice);
  }
  if (e == hipSuccess && B * W > 0) {
    hipLaunchKernelGGL(courant_reset_kernel, dim3(4), dim3(1024), 0, 0, (int)(B * W), op->d_ens_blk_max.p, op->d_ens_blk_pos.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return undo(fail(RDYHIP_ERR_LIB, "rdyhip_ensemble_enable: a device copy failed: %s", hipGetErrorString(e)));
  for (auto *b : bufs) op->device_bytes += (int64_t)b->bytes();
  op->device_bytes += (int64_t)(op->d_ens_blk_pos.bytes() + op->d_ens_courant.bytes());
  // The member groups.  Few cells: one group per member, down to ENSEMBLE_MIN_WORKGROUPS workgroups in all, so that a small
  // mesh still puts several workgroups on every CU; many cells: every thread walks up to ENSEMBLE_MAX_PER_GROUP members with
  // its geometry.
  const int64_t want = (ENSEMBLE_MIN_WORKGROUPS + (int64_t)std::max(op->grid, 1) - 1) / std::max(op->grid, 1);
  const int32_t g0   = (int32_t)std::min<int64_t>(num_members, std::max<int64_t>(want, 1));
  op->ens_per_group  = std::min((num_members + g0 - 1) / g0, ENSEMBLE_MAX_PER_GROUP);
  op->ens_groups     = (num_members + op->ens_per_group - 1) / op->ens_per_group;   // no group is empty
  op->ens_members    = num_members;
  op->ens_courant.assign(B, RDyHipCourant{0.0, -1, -1});
  return 0;
}

extern "C" int rdyhip_ensemble_info(RDyHipOperator op, int32_t *num_members) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (num_members) *num_members = op->ens_members;
  return 0;
}

extern "C" int rdyhip_ensemble_set_mannings(RDyHipOperator op, int32_t member, int32_t n, const int32_t *owned_cell_ids, const double *values) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  if (n > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  return scatter_component(op, op->d_ens_mannings.p + (size_t)member * (size_t)op->n_owned, 1, 0, n, owned_cell_ids, values);
}

extern "C" int rdyhip_ensemble_set_external_source(RDyHipOperator op, int32_t member, int32_t comp, int32_t n, const int32_t *owned_cell_ids,
                                                   const double *values) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  if (comp < 0 || comp > 2) return fail(RDYHIP_ERR_USER, "bad source component %d", comp);
  if (n > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  return scatter_component(op, op->d_ens_extsrc.p + (size_t)member * 3 * (size_t)op->n_owned, 3, comp, n, owned_cell_ids, values);
}

extern "C" int rdyhip_ensemble_set_boundary_values(RDyHipOperator op, int32_t member, int32_t boundary, int32_t num_edges, const double *values) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  int32_t off = 0, n = 0;
  rc = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  if (!values) return fail(RDYHIP_ERR_USER, "null values");
  HIP_TRY(hipDeviceSynchronize());   // an evaluation in flight on a non-blocking stream may still read the values this call replaces
  HIP_TRY(hipMemcpy(op->d_ens_bvalues.p + 3 * ((size_t)member * (size_t)op->K + (size_t)off), values, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int rdyhip_ensemble_rhs_function(RDyHipOperator op, const double *dts, const double *u_local, double *f_global, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!dts) return fail(RDYHIP_ERR_USER, "null dts");
  if (op->n_owned > 0 && (!u_local || !f_global)) return fail(RDYHIP_ERR_USER, "null u_local / f_global");
  return launch_ensemble(op, dts, u_local, f_global, nullptr, (hipStream_t)stream);
}

extern "C" int rdyhip_ensemble_euler_step(RDyHipOperator op, const double *dts, const double *u_local, double *u_local_out, double *f_global, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!dts) return fail(RDYHIP_ERR_USER, "null dts");
  if (op->n_owned > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");
  if (op->n_owned > 0 && (!u_local_out || u_local_out == u_local))
    return fail(RDYHIP_ERR_USER, "rdyhip_ensemble_euler_step needs a second state array (not in place)");
  return launch_ensemble(op, dts, u_local, f_global, u_local_out, (hipStream_t)stream);
}

extern "C" int rdyhip_ensemble_get_boundary_fluxes(RDyHipOperator op, int32_t member, int32_t boundary, int32_t num_edges, double *fluxes) {
  int rc = ensemble_check_member(op, member);
  if (rc) return rc;
  int32_t off = 0, n = 0;
  rc = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  if (!fluxes) return fail(RDYHIP_ERR_USER, "null output");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(fluxes, op->d_ens_bflux.p + 3 * ((size_t)member * (size_t)op->K + (size_t)off), sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rdyhip_ensemble_update_diagnostics(RDyHipOperator op, void *stream) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  const int B = op->ens_members;
  hipLaunchKernelGGL(ensemble_courant_finalize_kernel, dim3(B), dim3(BLOCK), 0, (hipStream_t)stream, ENSEMBLE_WAVES * op->grid, op->d_ens_blk_max.p,
                     op->d_ens_blk_pos.p, op->d_ens_courant.p);
  HIP_TRY(hipGetLastError());
  DeviceCourant dc[RDYHIP_MAX_ENSEMBLE_MEMBERS];
  HIP_TRY(hipMemcpyAsync(dc, op->d_ens_courant.p, sizeof(DeviceCourant) * (size_t)B, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  for (int m = 0; m < B; ++m) op->ens_courant[m] = courant_from_device(op, dc[m]);
  return 0;
}

extern "C" int rdyhip_ensemble_get_diagnostics(RDyHipOperator op, RDyHipCourant *courant) {
  int rc = ensemble_check(op);
  if (rc) return rc;
  if (!courant) return fail(RDYHIP_ERR_USER, "null argument");
  for (int m = 0; m < op->ens_members; ++m) courant[m] = op->ens_courant[m];
  return 0;
}
