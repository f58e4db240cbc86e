// MI355X-native SWE right-hand-side operator: the one translation unit of the library.  Here: create / destroy, the launch
// selection and the thin entry points of the C ABI declared in include/rdyhip.h; the mesh repack is host_layout.h, the
// operator's state operator_state.h, the setters field_io.h, the ghost exchange halo_*.h, and every feature on top of the RHS
// (RK4, output means, time series, read-out, tracers and their output, ensembles) its own *_calls.h.  gfx950 only.
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
#include "normal_table.h"
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
#include "tracer_output_kernels.h"
#include "ensemble_kernels.h"
#include "ens_output_kernels.h"
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

// ... and std::integral_constant<int, NT> for an operator's number of tracers, 1..7 (checked by the enable calls)
template <class F>
auto with_tracer_count(int nt, F f) {
  switch (nt) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    default: return f(std::integral_constant<int, 7>());
  }
}

// The instantiation of the tiled kernel for (slots per cell, source method, f = rhs (else f += rhs), HR, the forward-Euler update
// fused into the stores (rdyhip_euler_step; always f = rhs), F -- Euler step: u_out -- stored with the non-temporal hint,
// normals from the operator's table (swe_rhs_ntab_kernel) instead of one streamed double per record)
TiledKernelFn tiled_kernel_fn(int S, int src, bool ovw, bool hr, bool euler, bool fnt, bool ntab) {
  return with_flag(S == 4, [&](auto quad) { return with_flag(src != 0, [&](auto xq) { return with_flag(hr, [&](auto hr_) {
    return with_flag(fnt, [&](auto nt) -> TiledKernelFn {
      constexpr int s = quad ? 4 : 3, x = xq ? 1 : 0;
      if (ntab) {
        if (euler) return swe_rhs_ntab_kernel<s, x, true, hr_, true, nt>;
        return ovw ? swe_rhs_ntab_kernel<s, x, true, hr_, false, nt> : swe_rhs_ntab_kernel<s, x, false, hr_, false, nt>;
      }
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

// the Euler-step calls store u_out while neighbours still read u
int euler_out_check(RDyHipOperator op, const char *call, const double *u, const double *u_out) {
  if (op->n_owned > 0 && (!u_out || u_out == u)) return fail(RDYHIP_ERR_USER, "%s needs a second state array (not in place)", call);
  return 0;
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
  KernelArgs a = kernel_args_base(op);
  a.phase      = phase;
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
  if (reset_diag) op->courant_owned_side = false;
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
  KernelArgs a = kernel_args_base(op);
  a.u_out      = u_out;
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
      const bool     ntab   = op->ntab_entries > 0;  // fixed at create: d_e_lr carries the indices, the cold block the entries
      TiledKernelFn  kfn    = tiled_kernel_fn(op->S, xq ? 1 : 0, overwrite != 0, op->hr, euler_fused, !cached, ntab);
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
      hipLaunchKernelGGL(HIP_KERNEL_NAME(kfn), dim3(grid), dim3(TILE), ntab ? op->ntab_lds_bytes : op->lds_bytes, st, a, dt, u, f);
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
  // The normal table, for the operators that launch the first-order / HR tiled kernels: on the copy of the records that is
  // uploaded below (the layout pass and rdyhip_probe_layout know nothing of it).  Where the mesh has too many normals the words
  // stay as they are and the operator streams.
  NormalTable ntab;
  if (op->use_tiled && !op->muscl && !(config->flags & RDYHIP_CONFIG_STREAMED_NORMALS))
    ntab = build_normal_table(L.e_lr.data(), L.e_cs.data(), std::min(L.e_lr.size(), L.e_cs.size()));
  op->ntab_entries   = ntab.active ? (int32_t)ntab.cs.size() : 0;
  op->ntab_lds_bytes = tiled_ntab_lds_bytes(S, op->hr);
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
    const bool  nt  = op->ntab_entries > 0;
    const void *kfn = (const void *)tiled_kernel_fn(S, xq, true, op->hr, false, true, nt);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kfn, TILE, nt ? op->ntab_lds_bytes : op->lds_bytes) == hipSuccess && q > 0) per_cu = q;
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
    c.nt_count  = op->ntab_entries;
    for (int32_t i = 0; i < op->ntab_entries; ++i) {
      c.nt_cs[i]    = ntab.cs[i];
      c.nt_flags[i] = ntab.flags[i];
    }
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
  if (nc > no) {
    op->h_owned.resize(nc);
    for (size_t c = 0; c < nc; ++c) op->h_owned[c] = mesh->cell_is_owned[c] ? 1 : 0;
  }
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
  if (int rc = euler_out_check(op, "rdyhip_euler_step", u_local, u_local_out)) return rc;
  const int reset = (flags & RDYHIP_PHASE_RESET_DIAGNOSTICS) ? 1 : 0;
  if (reset) op->courant = RDyHipCourant{0.0, -1, -1};
  if (reset && phase == RDYHIP_PHASE_HALO && (op->use_tiled ? op->n_halo_tiles == 0 : op->n_halo == 0)) {
    int rc = rdyhip_reset_diagnostics(op, stream);
    if (rc) return rc;
  }
  return launch_rhs(op, phase, 1, reset, dt, u_local, f_global, (hipStream_t)stream, (flags & RDYHIP_PHASE_GRADIENTS_READY) != 0, u_local_out);
}

int rdyhip_get_boundary_fluxes(RDyHipOperator op, int32_t boundary, int32_t accumulated, int32_t num_edges, double *fluxes) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  return boundary_rows_copy(op, boundary, num_edges, accumulated ? op->d_baccum.p : op->d_bflux.p, 3, fluxes, false);
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

int rdyhip_normal_table_info(RDyHipOperator op, int32_t *entries, int32_t *active) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (entries) *entries = op->ntab_entries;
  if (active) *active = op->ntab_entries > 0 ? 1 : 0;
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
  op->courant_owned_side = false;
  return 0;
}

// the device's (value, position in the reference's loop order) as the value and the global ids of its edge and cell.
// owned_side: the number comes from a kernel that looks at a cut edge from its owned cell only, with len / area_self (tracers,
// ensembles: include/rdyhip.h); the cell of such an edge is then the owned one, whatever the area of the ghost behind it
static RDyHipCourant courant_from_device(RDyHipOperator op, const DeviceCourant &dc, bool owned_side = false) {
  RDyHipCourant out{dc.max_courant, -1, -1};
  if (dc.pos >= 0) {
    int32_t edge, cell;
    if (dc.pos < op->n_internal) {
      edge             = op->h_internal_edge[dc.pos];
      const int32_t l  = op->h_edge_cells[2 * (size_t)edge], r = op->h_edge_cells[2 * (size_t)edge + 1];
      cell             = (op->h_area[l] < op->h_area[r]) ? l : r;  // swe_petsc.c:294-295
      if (owned_side && !op->h_owned.empty()) {
        if (!op->h_owned[l]) cell = r;
        else if (!op->h_owned[r]) cell = l;
      }
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

// A non-blocking read (diagnostics_calls.h) that nobody waited for is given up: work enqueued on `st` from here on runs behind
// its copy, which may still be reading the device record from another stream
static int diagnostics_read_discard(DiagnosticsRead &r, hipStream_t st) {
  if (r.state == DiagnosticsRead::IN_FLIGHT) HIP_TRY(hipStreamWaitEvent(st, r.done, 0));
  r.state = DiagnosticsRead::NONE;
  return 0;
}

int rdyhip_update_diagnostics(RDyHipOperator op, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (int rc = diagnostics_read_discard(op->diag_read[RDYHIP_DIAGNOSTICS_OPERATOR], (hipStream_t)stream)) return rc;
  // the RHS launches keep one running (max, first position) bucket per workgroup slot; they are merged only here
  hipLaunchKernelGGL(courant_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (int)op->d_blk_max.n, op->d_blk_max.p, op->d_blk_pos.p,
                     op->d_courant.p);
  HIP_TRY(hipGetLastError());
  DeviceCourant dc;
  HIP_TRY(hipMemcpyAsync(&dc, op->d_courant.p, sizeof(dc), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  op->courant = courant_from_device(op, dc, op->courant_owned_side);
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
  fill_layout_info(*op, op->use_tiled, op->muscl ? op->pgrid_muscl : op->pgrid, op->device_bytes + op->feature_bytes(), info);
  return 0;
}

}  // extern "C"

#include "halo_exchange.h"
#include "halo_plan.h"
#include "rk_calls.h"
#include "output_shared.h"
#include "output_calls.h"
#include "series_calls.h"
#include "readout_calls.h"
#include "tracer_calls.h"
#include "tracer_output_calls.h"
#include "ensemble_calls.h"
#include "ens_output_calls.h"
#include "diagnostics_calls.h"

