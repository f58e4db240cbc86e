// HIP kernels of the SWE right-hand side for gfx950 (wave64, 160 KB LDS per CU).
//
// Two implementations of the same operator share the epilogue and the
// Courant reduction:
//
//  * swe_rhs_tiled_kernel (default): one workgroup = one tile of up to 256
//    consecutive owned cells (cut at create so that a tile's edge records and
//    halo cells fit fixed capacities: host_layout.h, layout_build_tiles).
//      phase 0  every thread loads its cell's state, derives the Riemann side
//               data (velocities, sqrt(h), sqrt(g h)) once and stages it in LDS;
//      phase 1  threads sweep the tile's edge list (every edge that touches a
//               tile cell, built at setup): left/right states come from LDS
//               (or from global memory for the few cells outside the tile),
//               each Roe flux is evaluated ONCE and parked in LDS;
//      phase 2  every thread sums its cell's <= S edge fluxes from LDS in the
//               reference's loop order (a segmented reduction with no
//               atomics), applies the source terms and writes F and the
//               primitive variables.
//    Edges cut by a tile boundary are evaluated by both tiles (bitwise
//    identically), so no inter-workgroup communication is needed.
//
//  * swe_rhs_kernel (RDYHIP_KERNEL=cell): one thread = one cell, every edge of
//    the cell evaluated by that thread (each interior edge twice overall).
//    Kept as the simple reference point for A/B measurements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdyhip.h"
#include "swe_device.h"

namespace rdyhip {

// (BLOCK, TILE, the capacities every tile is cut to, the packed edge records and TileDesc: tile_format.h)

// Data that is streamed through exactly once per launch -- the per-cell streams (flux coefficients, bed slopes,
// Manning n, external source), the tile edge records and the outputs F / primitive variables -- is loaded and
// stored with the non-temporal hint, which leaves the L2 to the state vector (the only data with reuse: halo cells
// are read by neighbouring tiles).  Measured A/B on one box: 0.342 ms vs 0.359 ms per 10 M-cell RHS; marking the
// state loads as well costs 5 % (0.375 ms), the stores alone cost 6 %.
#define RDY_ST(ptr, val) __builtin_nontemporal_store((val), (ptr))
#define RDY_LD(ptr) __builtin_nontemporal_load(ptr)

// persistent Courant diagnostic on the device
struct DeviceCourant {
  double  max_courant;
  int32_t pos;  // position of the edge in the reference's loop order, -1 = none
  int32_t pad;
};

// Kernel arguments.  A wave has 102 SGPRs; the persistent tiled kernels keep three tile descriptors, the loop state and
// every pointer their hot path reads in them for the whole launch.  Whatever only rare paths read -- the boundary-edge
// tables (a few boundary edges per tile at most), the Courant tie-break positions and the per-workgroup buckets (once per
// workgroup), the cell-centric kernel's neighbour tables -- lives in a device-resident ColdArgs block, written once at
// create and read through ONE pointer with scalar loads at the point of use (RDY_COLD), so that it occupies no register
// on the hot path.  (Round 2 passed all ~40 pointers by value: 51-83 SGPRs spilled to VGPR lanes per instantiation.)
struct ColdArgs {
  const int32_t *nbr;        // [S][stride] neighbour ids (cell kernel, gradient kernel)
  const double  *cn, *sn;    // [S][stride] (cell kernel)
  const int32_t *pos;        // [S][stride] loop position of each slot's edge (Courant tie-break of the cell kernel)
  const int32_t *e_pos;      // [nrec + n_xedges] loop position of each tile edge record (Courant tie-break of the tiled kernels),
                             //                   then of each extra Courant edge
  // Internal edges of the local mesh that no owned cell's slot covers the way the reference's loop does (swe_petsc.c:275-296
  // runs over ALL local internal edges and divides by min(area_l, area_r) whoever owns the cells): edges between two ghost
  // cells, and owned / ghost edges whose ghost cell is the smaller one.  O(cut edges); evaluated -- the largest wave speed only --
  // by the threads of a launch that has ghost data (courant_extra_edges), so that a rank's Courant diagnostic BEFORE the
  // cross-rank reduction is the reference's, ties and all.
  int32_t        n_xedges;
  int32_t        x_rec0;     // = nrec: extra edge i is "record" x_rec0 + i of e_pos
  const int32_t *x_lr;       // [n_xedges][2] local ids of the left / right cell
  const uint32_t *x_flags;   // [n_xedges] EDGE_CS_IS_CN | EDGE_OTHER_NEG of the packed normal
  const double  *x_cs;       // [n_xedges] its stored component
  const double  *x_cfac;     // [n_xedges] len / min(area_l, area_r)
  const double  *x_mid;      // [n_xedges][2] edge midpoint (second order)
  const int32_t *btype;      // [K] condition type of boundary edge k
  const double  *bvalues;    // [K][3]
  double        *bflux;      // [K][3]
  double        *baccum;     // [K][3]
  const int32_t *tile_bk;    // boundary-edge ids k of each tile's boundary edges
  const int32_t *tile_boff;  // [ntiles + 1] first tile_bk entry of each tile
  double        *blk_max;    // [2 * maxgrid] the Courant diagnostic, one running (max, first position) bucket per workgroup slot;
  int32_t       *blk_pos;    //               merged by courant_finalize_kernel only when the host asks (rdyhip_update_diagnostics)
  // the pack of the next ghost update fused into the Euler-step kernels' stores (rdyhip_halo_fuse_pack): tiles flagged
  // TILE_SEND_FLAG also store the new state of their send cells into the halo's send buffer
  const int32_t  *send_off;  // [ntiles + 1] first send entry of each tile
  const uint32_t *send_ent;  // cell-in-tile (bits 0-7) | row of the send buffer (bits 8-31), sorted by tile
  double         *send_buf;  // [send cells][3]
  // second order: the ghost-adjacent cells' gradient launch (muscl_gradient_kernel over the halo cell list) also stores each
  // gradient into the rows of the send buffer that carry it to other ranks: no pack launch for the gradient exchange
  const int32_t *gsend_off;   // [n_halo + 1] first send row of the cell at each position of the halo cell list
  const int32_t *gsend_rows;  // rows of the send buffer ([send cells][6])
  double        *gsend_buf;
  // The dynamic tile walk of the first-order / HR tiled kernels (KernelArgs::tile_walk): counters 0-7 count the tiles drawn
  // from each XCD's range beyond the workgroups' static ones, counter 8 the workgroups that have left.  Zero between launches:
  // the workgroup that leaves last zeroes all nine, and the next launch that uses them is ordered behind it on the stream.
  // One counter per TILE_DRAW_STRIDE words: side by side in one cache line the eight XCDs' draws queue for that line like
  // draws from ONE counter (measured: the launch took 1.9 x as long, profiles/RESULTS_LOG.md section 21).
  int32_t       *tile_draw;  // [9 * TILE_DRAW_STRIDE]
  // The normal table of the table kernels (swe_rhs_ntab_kernel; normal_table.h): nt_count entries, 0 where the operator
  // streams its normals.  Each workgroup turns them into (cn, sn) pairs in LDS once, with edge_normal; bits 26-31 of a
  // record's e_lr word say which entry is the record's.  (At the end: every field above keeps its offset.)
  int32_t        nt_count;
  int32_t        nt_pad;
  double         nt_cs[NORMAL_TABLE_MAX];     // the stored component
  uint32_t       nt_flags[NORMAL_TABLE_MAX];  // EDGE_CS_IS_CN | EDGE_OTHER_NEG, where a record's word has them
};
constexpr int TILE_DRAW_STRIDE = 64;  // 256 B
constexpr int TILE_WALK_MIN_ROUNDS = 32;  // tiles per workgroup from which a launch walks dynamically by default (launch_rhs)

enum { TILE_WALK_STATIC = 0, TILE_WALK_DYNAMIC = 1, TILE_WALK_STATIC_SKIP = 2 };
struct KernelArgs {
  int32_t        n_owned;    // owned cells
  int32_t        n_work;     // cell kernel: threads with work; tiled kernel: number of tiles to run
  int64_t        stride;     // distance between slot planes
  const int32_t *list;       // cell kernel: owned-cell ids; tiled kernel: tile ids; or nullptr for 0..n_work-1
  const int32_t *o2l;        // owned -> local cell id, or nullptr if the identity
  const double  *coef;       // [S][stride]
  const double  *dzdx, *dzdy;  // [n_owned]
  const double  *mannings;   // [n_owned]
  const double  *extsrc;     // src_mom = 1: [n_owned][3]; src_mom = 0: [n_owned], the water component alone
  double        *pv;         // [n_owned][3] or nullptr: nobody has asked for the primitive variables, they are not stored
  double        *fdiv;       // [n_owned][3] or nullptr
  double        *u_out;      // EULER kernels: [num_cells][3] state after the step, owned rows written (u_out = u + dt F)
  const ColdArgs *cold;      // device memory: see above
  int32_t        bucket_off; // first Courant bucket of this launch (launch_rhs(bucket_half))
  int32_t        n_buckets;
  int32_t        reset_diag; // 1: this launch starts a new diagnostic (ResetOperatorDiagnostics): buckets are overwritten
  int32_t        tile_walk;  // first-order / HR tiled kernel, TILE_WALK_*: DYNAMIC: after its first tile a workgroup draws its
                             // tiles from its XCD's counter (ColdArgs::tile_draw), set by launch_rhs for PHASE_ALL launches with
                             // xcd_chunks > 0 only; STATIC_SKIP: the static walk of an INTERIOR phase, which skips tiles (phase
                             // says the same: the tile loop reads this one word for both).  (Sits in what was padding, like src_mom.)
  double         tiny_h, h_anuga_sq, xq_thresh;
  int32_t        phase;      // RDYHIP_PHASE_*
  int32_t        overwrite;  // 1: f = rhs, 0: f += rhs
  int32_t        xcd_chunks; // >0: blocks are dealt to XCDs in contiguous chunks of this many tiles
  int32_t        src_mom;    // first-order / HR tiled kernel, STREAM_* bits.  Bit 0 set: extsrc holds all three source components;
                             // clear: extsrc is the dense water-source plane and the momentum sources are zero (launch_rhs).  Bits 1-3:
                             // the water source / Manning's n / the bed slopes are uniform over the owned cells, element 0 stands for
                             // all of them (stream_args).  The other kernels always get the [n_owned][3] array and 1, and do not look.
                             // (Sits in what was padding: the struct does not grow.)
  // ---- tiled kernel only
  const struct TileDesc *tiles;  // [ntiles+1]
  const uint32_t *e_lr;      // [nrec] packed LDS slots of the edge's cells
  const double   *e_cs;      // [nrec] smaller-magnitude component of the edge normal
  const int32_t  *hcells;    // halo cells of each tile (local cell ids)
  const void     *slot_ref;  // index of each slot's edge in the tile's edge list: S == 3: uint32[n_owned] (3 x 10 bits),
                             // S == 4: uint16[n_owned][4]
  const double   *zc_local;  // [num_cells] vertex-averaged bed elevation (hydrostatic reconstruction only)
};

// Wave-uniform loads of read-only index data through the constant address space,
// so that hipcc emits scalar loads (s_load, counted by lgkmcnt) instead of vector
// loads whose s_waitcnt vmcnt(0) would also wait for every prefetch in flight.
template <typename T>
__device__ __forceinline__ T load_uniform(const T *p, int i) {
  typedef const __attribute__((address_space(4))) T *ConstPtr;
  return ((ConstPtr)(uintptr_t)p)[i];
}

// Unit-stride accesses of the tiled kernels: element (wave-uniform index) + (lane) of an array, as a 64-bit SCALAR base -- the
// array plus the uniform part, made with scalar adds next to the access -- and a 32-bit lane offset in bytes that does not change
// from tile to tile (4 tid, 8 tid, the row offset of the store phase): `global_load v, v_off, s[base:base+1]`.  Written as
// array[uniform + lane], hipcc builds the 64-bit address per lane and per tile instead (a move of each scalar half into a VGPR,
// a sign extension, a 64-bit shift-and-add: two to three VALU instructions per access).  The base goes through an empty asm:
// otherwise the optimiser folds base + lane back into one 64-bit lane index.  As a GLOBAL address: through a generic pointer
// the access becomes a flat one, which every lgkmcnt wait -- scalar loads, LDS -- then waits for as well.
//      The "+s" operand needs a base that hipcc can PROVE wave-uniform.  Where it cannot -- every base here is uniform, but an
// unrelated edit can hide that from the divergence analysis: a single `if (threadIdx.x == 0)` store at kernel entry (the probe,
// tools/probes/wg_times.patch) does, in the 44 instantiations without the dynamic walk -- the compile fails, loudly, with
// "illegal VGPR to SGPR copy" reported at the kernel's signature.  The measured fallback is one line ahead of the asm:
//   b = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32);
// (the builtin returns a SIGNED int: without the uint32_t casts the low half is sign-extended over the high one and every base
// with bit 31 set is a wild address).  It compiles everywhere and leaves the C3 kernel as it is (797 loop VALU), but costs the
// Euler-step kernels of that family 18 VALU-issued instructions per tile (826 -> 844: 40 more lane operations in the kernel),
// so it is not in the product (profiles/RESULTS_LOG.md section 27).
template <typename T>
using GlobalPtr = __attribute__((address_space(1))) T *;
template <typename T>
__device__ __forceinline__ GlobalPtr<T> lane_ptr(T *uniform_base, uint32_t lane_bytes) {
  uint64_t b = (uint64_t)uniform_base;
  asm("" : "+s"(b));
  return (GlobalPtr<T>)(b + lane_bytes);
}
// The lane offset tid << log2(bytes), made where it is used from a shift count the optimiser cannot see: as a loop-invariant
// value it is hoisted out of the tile loop with its zero-extension -- a VGPR pair per offset held for the launch, and a 64-bit
// vector add per access again, because the extension is no longer in the block of the access.
__device__ __forceinline__ uint32_t lane_bytes(int tid, int log2_bytes) {
  asm volatile("" : "+s"(log2_bytes));
  return (uint32_t)tid << log2_bytes;
}

// a field of the device-resident ColdArgs block: one scalar load at the point of use
#define RDY_COLD(a, field) (load_uniform(&(a).cold->field, 0))

// The explicit arguments of the tiled kernel as they lie in its kernarg segment.  Pointers that the tile loop uses once per tile
// (the per-cell stream arrays, the output arrays, u) are fetched from there with scalar loads where they are used (RDY_HOT), a
// whole group per s_load, instead of being kept in SGPRs across the loop: held for the launch they do not fit beside the three
// tile descriptors and the loop state, hipcc spills them to VGPR lanes and restores them -- sixteen at a time, one VALU
// instruction per register -- in the middle of the blocks that issue the loads (profiles/RESULTS_LOG.md section 16).  The
// segment's address goes through an empty asm once per use site: a new value per tile as far as the optimiser knows, so the
// loads stay where they are written instead of being hoisted out of the loop and spilled again.
struct TiledKernargs {
  KernelArgs    a;
  double        dt;
  const double *u;
  double       *f;
};
typedef const __attribute__((address_space(4))) TiledKernargs *HotArgs;
__device__ __forceinline__ HotArgs hot_kernargs() {
  uint64_t p = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return (HotArgs)p;
}

// The workgroup's block of cells in the cell-centric kernels.  Block ids are dealt round-robin to the 8 XCDs: with
// xcd_chunks > 0 (KernelArgs) each XCD gets a contiguous range of blocks, so concurrently running blocks are neighbours.
// (Takes the count, not the KernelArgs: read through a reference here, it moves the kernels' code.)
__device__ __forceinline__ int xcd_block(int xcd_chunks) {
  return xcd_chunks > 0 ? (blockIdx.x & 7) * xcd_chunks + (blockIdx.x >> 3) : blockIdx.x;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}

// Source terms of a cell on its in-register flux sum (acc1, acc2): the bed slope g h dz/dx, g h dz/dy and the friction
// (tbx, tby) of ApplySourceSemiImplicit / ApplySourceImplicitXQ2018 (src/swe/swe_petsc.c:704-804, 816-932); the source reads
// the pre-source F (src/operator.c:663).
template <int SRC>
__device__ __forceinline__ void cell_source(const KernelArgs &a, double dt, double h, double hu, double hv, double acc1, double acc2, double dzdx,
                                            double dzdy, double n, double &bedx, double &bedy, double &tbx, double &tby) {
  bedx = dzdx * GRAVITY * h;
  bedy = dzdy * GRAVITY * h;
  tbx = tby = 0.0;
  if (h >= a.tiny_h) {
    if (SRC == RDYHIP_SOURCE_SEMI_IMPLICIT) friction_semi_implicit(h, hu, hv, n, dt, acc1, acc2, bedx, bedy, tbx, tby);
    else friction_xq2018(h, hu, hv, n, dt, a.xq_thresh, acc1, acc2, bedx, bedy, tbx, tby);
  }
}

// F of a cell, then the stores of F and the primitive variables (the cell-centric kernel).  F is summed after the fdiv
// stores, not taken from cell_results: computed ahead of that branch it moves the kernel's code.
template <int SRC>
__device__ __forceinline__ void cell_epilogue(const KernelArgs &a, int o, double dt, double h, double hu, double hv, double pu, double pv_, double acc0,
                                              double acc1, double acc2, double dzdx, double dzdy, double n, double s0, double s1, double s2,
                                              double *__restrict__ f) {
  double bedx, bedy, tbx, tby;
  cell_source<SRC>(a, dt, h, hu, hv, acc1, acc2, dzdx, dzdy, n, bedx, bedy, tbx, tby);
  if (a.fdiv) {
    a.fdiv[3 * (int64_t)o + 0] = acc0;
    a.fdiv[3 * (int64_t)o + 1] = acc1;
    a.fdiv[3 * (int64_t)o + 2] = acc2;
  }
  f[3 * (int64_t)o + 0] = acc0 + s0;
  f[3 * (int64_t)o + 1] = acc1 + (-bedx - tbx + s1);
  f[3 * (int64_t)o + 2] = acc2 + (-bedy - tby + s2);
  // primitive variables (swe_petsc.c:788-791): the regularised velocities of the Riemann states, zero below tiny_h
  // (stored once somebody has asked for them: KernelArgs::pv)
  if (a.pv) {
    a.pv[3 * (int64_t)o + 0] = h;
    a.pv[3 * (int64_t)o + 1] = pu;
    a.pv[3 * (int64_t)o + 2] = pv_;
  }
}

// F of a cell into out[3], for the tiled kernels (they store whole rows per wave: wave_store_rows3)
template <int SRC>
__device__ __forceinline__ void cell_results(const KernelArgs &a, double dt, double h, double hu, double hv, double acc0, double acc1, double acc2,
                                             double dzdx, double dzdy, double n, double s0, double s1, double s2, double *out) {
  double bedx, bedy, tbx, tby;
  cell_source<SRC>(a, dt, h, hu, hv, acc1, acc2, dzdx, dzdy, n, bedx, bedy, tbx, tby);
  out[0] = acc0 + s0;
  out[1] = acc1 + (-bedx - tbx + s1);
  out[2] = acc2 + (-bedy - tby + s2);
}
// Stores one [cell][3] row per lane of a full wave, transposed so that the wave writes its 192 consecutive doubles
// with three unit-stride instructions.  `base`: index of the wave's first double; lanes >= ncell hold no cell.
// NT = false: store with the default cache policy instead of the non-temporal hint -- F when a separate update kernel reads it
// straight back (TSEULER's VecAXPY: RDYHIP_CONFIG_CACHED_F_STORES).  A COMPILE-TIME choice on purpose: round 4 first made it a
// wave-uniform run-time branch around the store, and the optimiser sank the two arms (same value, same address) into ONE store
// whose metadata is the intersection of the two -- the hint was dropped from every F / pv / u_out store of every kernel, first
// order -6 %, and nothing but a same-box A/B against the previous round's library showed it (tests/test_isa_cpu.py now counts
// the hinted stores of every RHS kernel in the built library).
template <bool NT = true>
__device__ __forceinline__ void wave_store_rows3(double *__restrict__ arr, int64_t base, int lane, int ncell, double v0, double v1, double v2) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int    e = 64 * k + lane, src = e / 3, comp = e - 3 * src;
    const double s0 = __shfl(v0, src, 64), s1 = __shfl(v1, src, 64), s2 = __shfl(v2, src, 64);
    if (src < ncell) {
      if (NT) RDY_ST(&arr[base + e], comp == 0 ? s0 : (comp == 1 ? s1 : s2));
      else arr[base + e] = comp == 0 ? s0 : (comp == 1 ? s1 : s2);
    }
  }
}

// The same stores with the transpose done through 192 doubles of LDS that belong to the wave alone at that point, instead of
// nine 64-bit shuffles (18 ds_bpermute_b32) and a three-way select per stored value: lane l writes its row to elements
// 3 l .. 3 l + 2, then reads elements l, 64 + l, 128 + l.  `wr`: the lane's three write slots, `rd`: element `lane`; the
// elements are 64-entry pieces of three planes a fixed distance `plane` apart (the tiled kernel passes its own cells' entries
// of sd_v, sd_sq and sd_c: phase 1 was their last reader, before the second barrier; the wave itself rewrites them in phase 0
// of its next tile).  LDS serves a wave's instructions in order, so a read returns what the write before it stored; the
// wave-scope fences only keep the compiler from reordering the two across lanes' addresses it cannot tell apart.
struct RowTranspose {
  double *wr[3];
  double *rd;
};
template <int PLANE>
__device__ __forceinline__ RowTranspose row_transpose_slots(double *wave_plane0, int lane) {
  RowTranspose t;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int e = 3 * lane + j;
    t.wr[j]     = wave_plane0 + (e >> 6) * PLANE + (e & 63);
  }
  t.rd = wave_plane0 + lane;
  return t;
}
// `rows`: the array at the TILE's first row, wave-uniform; `row_bytes`: where the lane's element of the wave's first 64 lies
// behind it, 8 (3 (tid - lane) + lane) -- a scalar base and a 32-bit lane offset (lane_ptr), the three stores 512 B apart.
template <int PLANE, bool NT = true>
__device__ __forceinline__ void wave_store_rows3_lds(double *rows, uint32_t row_bytes, int lane, int ncell, const RowTranspose &t, double v0, double v1,
                                                     double v2) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the reads of the array before this one come first
  __builtin_amdgcn_wave_barrier();
  *t.wr[0] = v0;
  *t.wr[1] = v1;
  *t.wr[2] = v2;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const double s0 = t.rd[0], s1 = t.rd[PLANE], s2 = t.rd[2 * PLANE];
  // element 64 k + lane belongs to cell (64 k + lane) / 3 of the wave: stored if that cell exists, i.e. 64 k + lane < 3 ncell
  // (the address is formed under each predicate: formed once ahead of the three, it is a 64-bit vector add and a VGPR pair)
  const int e = 3 * ncell - lane;
  if (NT) {
    if (e > 0) RDY_ST(lane_ptr(rows, row_bytes), s0);
    if (e > 64) RDY_ST(lane_ptr(rows, row_bytes) + 64, s1);
    if (e > 128) RDY_ST(lane_ptr(rows, row_bytes) + 128, s2);
  } else {
    if (e > 0) *lane_ptr(rows, row_bytes) = s0;
    if (e > 64) lane_ptr(rows, row_bytes)[64] = s1;
    if (e > 128) lane_ptr(rows, row_bytes)[128] = s2;
  }
}

// What a lane WITHOUT a cell carries into the store phase.  It takes part in the wave's transpose like every other lane, and
// the rows it writes there are masked at the store (wave_store_rows3_lds: element e is stored only if its cell exists; the
// scattered u_out rows sit under the lane's own `active`), so the values are read by nobody.  They are whatever the registers
// hold: an empty asm names them as its outputs, which defines them for the compiler without an instruction -- zeroing them
// cost the tile loop eighteen 32-bit registers' worth of moves per tile.
__device__ __forceinline__ void rows_unset(double (&out)[6], double (&acc)[3], double &hu, double &hv) {
  asm volatile("" : "=v"(out[0]), "=v"(out[1]), "=v"(out[2]), "=v"(out[3]), "=v"(out[4]), "=v"(out[5]), "=v"(acc[0]), "=v"(acc[1]), "=v"(acc[2]),
               "=v"(hu), "=v"(hv));
}

// A thread's running Courant maximum over the tiles it walks (swe_petsc.c:289-296: the reference keeps the FIRST edge in
// loop order that reaches the maximum).  Inside one cell the slots are in loop order, so "strictly greater" keeps the
// first; across the cells a thread visits nothing orders the loop positions (DMPlex numbers edges on its own,
// src/rdymesh.c:693-710).  The hot path only NOTES that a slot met the running maximum to the last bit (one compare per
// slot, the flag lives in a scalar mask); a cell that did goes through courant_resolve_tie -- cold code, taken by states
// that are uniform over what a thread has seen so far (a lake at rest, the flat pools of the reference's dam-break
// benchmark at t = 0) -- which compares loop positions.  That path must be cheap too (the dam break's first steps run
// through it in every tile): the incumbent's position is looked up once and kept; a candidate whose position is known
// to be larger is dismissed without touching memory -- the records of a tile are sorted by position, so the position of
// record 0 bounds every candidate of the tile from below and that of record COURANT_Q bounds the candidates from
// record COURANT_Q on (two scalars per tile, fetched a tile ahead; where the edge numbering follows the cells the first
// few dozen records of a tile are the edges it shares with earlier tiles, everything behind them is newer than any
// incumbent); otherwise one 4-byte load per tying cell, waited for inside the branch.
constexpr int COURANT_Q = 48;
struct CourantTrack {
  double best = 0.0;  // largest Courant number seen by this thread (> 0 only)
  int    rec  = 0;    // its tile edge record (index into e_lr / e_cs / e_pos)
  int    pos  = -1;   // the loop position of `rec` once a tie has made the thread look it up
};
// rec_new: the record of the FIRST slot of the current cell that equals t.best; tile_pos_lo: the smallest loop position among the
// current tile's records
__device__ __forceinline__ void courant_resolve_tie(const KernelArgs &a, CourantTrack &t, int rec_new, int tile_pos_lo) {
  if (rec_new == t.rec) return;  // the incumbent is that very slot
  const int32_t *e_pos = RDY_COLD(a, e_pos);
  if (t.pos < 0) {
    int po = e_pos[t.rec];
    // waited for HERE: a load whose result is first used after the merge costs every wave an s_waitcnt vmcnt(0) at the
    // merge, and with it a wait for the next tile's prefetch batch
    asm volatile("" : "+v"(po));
    t.pos = po;
  }
  if (t.pos < tile_pos_lo) return;
  int pn = e_pos[rec_new];
  asm volatile("" : "+v"(pn));
  if (pn < t.pos) {
    t.rec = rec_new;
    t.pos = pn;
  }
}

// `table[index]`: the loop position of the thread's candidate (read only by the lanes that hold the block's maximum)
template <int NT>
__device__ __forceinline__ void block_courant_reduce(const KernelArgs &a, double best, const int32_t *table, int64_t index) {
  __shared__ double s_max[NT / 64];
  __shared__ int    s_pos[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double    wmax = wave_max(best);
  if (lane == 0) s_max[wave] = wmax;
  __syncthreads();
  double bmax = s_max[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) bmax = fmax(bmax, s_max[w]);
  int p = INT32_MAX;
  if (best > 0.0 && best == bmax) p = table[index];
  p = wave_min(p);
  if (lane == 0) s_pos[wave] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    int bp = s_pos[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) bp = min(bp, s_pos[w]);
    double m = bmax;
    int    q = (bmax > 0.0) ? bp : -1;
    const int b       = blockIdx.x;
    double   *blk_max = RDY_COLD(a, blk_max) + a.bucket_off;
    int32_t  *blk_pos = RDY_COLD(a, blk_pos) + a.bucket_off;
    if (!a.reset_diag) {  // merge into the bucket: larger value, then the earlier edge (swe_petsc.c:291 keeps the first)
      const double pm = blk_max[b];
      const int    pq = blk_pos[b];
      if (pm > m || (pm == m && pm > 0.0 && pq < q)) {
        m = pm;
        q = pq;
      }
    }
    blk_max[b] = m;
    blk_pos[b] = q;
    if (a.reset_diag) {  // buckets no workgroup of this launch owns
      for (int k = b + gridDim.x; k < a.n_buckets; k += gridDim.x) {
        blk_max[k] = 0.0;
        blk_pos[k] = -1;
      }
    }
  }
}

__device__ __forceinline__ void store_boundary_flux(const KernelArgs &a, int k, const RoeFlux &fl, double dt) {
  // boundary_fluxes[b] and VecAXPY(boundary_fluxes_accum, dt, boundary_fluxes), swe_petsc.c:574, 623
  double *bflux = RDY_COLD(a, bflux), *baccum = RDY_COLD(a, baccum);
  bflux[3 * (int64_t)k + 0] = fl.f0;
  bflux[3 * (int64_t)k + 1] = fl.f1;
  bflux[3 * (int64_t)k + 2] = fl.f2;
  baccum[3 * (int64_t)k + 0] += dt * fl.f0;
  baccum[3 * (int64_t)k + 1] += dt * fl.f1;
  baccum[3 * (int64_t)k + 2] += dt * fl.f2;
}

// ---------------------------------------------------------------------------
// tiled kernel (the packed edge records EDGE_*, REF3_EMPTY and the tile descriptor: tile_format.h)
// ---------------------------------------------------------------------------

// index of slot s's edge in the tile's edge list, or -1 for an unused slot.  r0 (, r1): the cell's slot references
// (KernelArgs::slot_ref): triangles three 10-bit ones in r0, quads four 16-bit ones in r0, r1.  (The first-order kernel's
// phase 2 decodes inline: through this function its quad instantiations compile to other code.)
template <int S>
__device__ __forceinline__ int slot_edge(uint32_t r0, uint32_t r1, int s) {
  if (S == 3) {
    const uint32_t ref = (r0 >> (10 * s)) & 0x3FF;
    return ref == REF3_EMPTY ? -1 : (int)ref;
  }
  const uint32_t w   = (s < 2) ? r0 : r1;
  const uint32_t ref = (s & 1) ? (w >> 16) : (w & 0xFFFFu);
  return ref == SLOT_EMPTY ? -1 : (int)ref;
}

__device__ __forceinline__ void edge_normal(uint32_t lr, double cs, double &cn, double &sn) {
  double other = rdy_sqrt(fma(-cs, cs, 1.0));
  if (lr & EDGE_OTHER_NEG) other = -other;
  const bool is_cn = lr & EDGE_CS_IS_CN;
  cn               = is_cn ? cs : other;
  sn               = is_cn ? other : cs;
}

// The fused pack: the lanes of a wave hand the new state of the tile's send cells to the send buffer.  Every wave scans the
// tile's (short) entry list 64 entries at a time and takes the entries whose cell it holds; the values come from the owning
// lane through a wave shuffle, so there is no LDS traffic and no barrier.  Runs only in tiles flagged TILE_SEND_FLAG.
__device__ __forceinline__ void wave_store_send_rows(const KernelArgs &a, int tile, int tid, double n0, double n1, double n2) {
  const int32_t  *soff = RDY_COLD(a, send_off);
  const int       s0 = load_uniform(soff, tile), s1 = load_uniform(soff, tile + 1);
  const uint32_t *sent = RDY_COLD(a, send_ent);
  double         *sbuf = RDY_COLD(a, send_buf);
  const int       lane = tid & 63, wave = tid >> 6;
  for (int base = s0; base < s1; base += 64) {
    const int      i   = base + lane;
    const uint32_t ent = i < s1 ? sent[i] : 0u;
    const int      j   = (int)(ent & 0xFFu);
    const double   v0 = __shfl(n0, j & 63, 64), v1 = __shfl(n1, j & 63, 64), v2 = __shfl(n2, j & 63, 64);
    if (i < s1 && (j >> 6) == wave) {
      const int64_t row = (int64_t)(ent >> 8);
      sbuf[3 * row + 0] = v0;
      sbuf[3 * row + 1] = v1;
      sbuf[3 * row + 2] = v2;
    }
  }
}

// per-cell streams consumed in phase 2 (slot references, flux coefficients,
// bed slopes, Manning n, external source)
template <int S>
struct CellStreams {
  uint32_t r0, r1;
  double   coef[S];
  double   dzdx, dzdy, nman, s0, s1, s2;
};

// The pointers and the scalars load_streams reads: filled from the kernarg segment where the streams are issued (RDY_HOT).
// KernelArgs::src_mom carries the launch's stream flags: STREAM_SRC_MOM, and one bit per field whose owned elements all hold
// the same 64-bit pattern at enqueue time (uniform_fields.h).  Each such bit becomes an index mask, 0 instead of -1, with
// scalar code: every lane of every wave then reads element 0 of the SAME array the setters keep current -- one line, always on
// chip, the same bits its own element holds -- and the field's plane costs the launch no HBM traffic.  Branch-free on purpose:
// a wave-uniform branch around each load costs the tile loop 11 VALU instructions and four hinted loads (profiles/RESULTS_LOG.md section 24).
enum { STREAM_SRC_MOM = 1, STREAM_UNIFORM_SOURCE = 2, STREAM_UNIFORM_MANNINGS = 4, STREAM_FLAT_BED = 8 };
struct StreamArgs {
  const void   *slot_ref;
  const double *coef, *dzdx, *dzdy, *mannings, *extsrc;
  int64_t       stride;
  int32_t       src_mom;
  int32_t       mask_s, mask_n, mask_dz;  // 0: the field is uniform, read element 0; -1: read the lane's own element
};
__device__ __forceinline__ StreamArgs stream_args(HotArgs k) {
  StreamArgs p;
  p.slot_ref = k->a.slot_ref;
  p.coef     = k->a.coef;
  p.dzdx     = k->a.dzdx;
  p.dzdy     = k->a.dzdy;
  p.mannings = k->a.mannings;
  p.extsrc   = k->a.extsrc;
  p.stride   = k->a.stride;
  const int32_t flags = k->a.src_mom;
  p.src_mom  = flags & STREAM_SRC_MOM;
  p.mask_s   = ((flags >> 1) & 1) - 1;
  p.mask_n   = ((flags >> 2) & 1) - 1;
  p.mask_dz  = ((flags >> 3) & 1) - 1;
  return p;
}

// Only the lanes that hold a cell load, and only they read `c` afterwards: phase 2 runs under the same count (tid < td.nc())
// and the arrival points name registers, not values.  The other lanes' registers are left as they are -- setting them cost
// ten moves per tile.
// The lane's cell is c_off + tid: every address is a scalar base (array + the tile's first cell, lane_ptr) plus the lane's
// 4 tid or 8 tid; a uniform field's mask (0 / -1) goes on both parts, so that every lane reads element 0.
template <int S, bool HR>
__device__ __forceinline__ void load_streams(const StreamArgs &a, int c_off, int tid, bool active, CellStreams<S> &c) {
  if (active) {
    const uint32_t t4 = lane_bytes(tid, 2), t8 = lane_bytes(tid, 3);
    const int64_t  o0 = c_off;
    if (S == 3) {
      c.r0 = RDY_LD(lane_ptr(reinterpret_cast<const uint32_t *>(a.slot_ref) + o0, t4));
    } else {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 w = *lane_ptr(reinterpret_cast<const u32x2 *>(a.slot_ref) + o0, t8);
      c.r0          = w.x;
      c.r1          = w.y;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) c.coef[s] = RDY_LD(lane_ptr(a.coef + (s * a.stride + o0), t8));
    if (!HR) {  // under HR the pressure correction of the flux carries the bed slope
      const int64_t  oz = c_off & a.mask_dz;
      const uint32_t tz = t8 & (uint32_t)a.mask_dz;
      c.dzdx = RDY_LD(lane_ptr(a.dzdx + oz, tz));
      c.dzdy = RDY_LD(lane_ptr(a.dzdy + oz, tz));
    } else {
      c.dzdx = c.dzdy = 0.0;
    }
    c.nman = RDY_LD(lane_ptr(a.mannings + (int64_t)(c_off & a.mask_n), t8 & (uint32_t)a.mask_n));
    // the water source: row o of the [owned][3] array, or entry o of the water plane, which costs 8 B of HBM traffic per cell
    // instead of the 24 B that any read of a 24-B row does -- or entry 0 of the plane where the source is uniform, which costs none
    // (one load for both forms, its base and the lane's stride chosen with scalar code)
    const int32_t  ms  = a.src_mom ? -1 : a.mask_s;
    const double  *src = a.extsrc + (a.src_mom ? 3 * o0 : (int64_t)(c_off & ms));
    const uint32_t ts  = ((a.src_mom ? 24u : 8u) * (uint32_t)tid) & (uint32_t)ms;
    c.s0 = RDY_LD(lane_ptr(src, ts));
    // (s1 / s2 of the water-only mode are the zeros `cur{}` starts with: nothing writes them again during such a launch)
    if (a.src_mom) {  // wave-uniform
      c.s1 = RDY_LD(lane_ptr(src, ts) + 1);
      c.s2 = RDY_LD(lane_ptr(src, ts) + 2);
    }
  }
}

// The two rounds of a tile's edge records, each under the count phase 1 tests; a lane without a record keeps what it has.
// The second round is the same lane offset against a base TILE records further on.
__device__ __forceinline__ void load_records(const KernelArgs &a, int e_off, int ne, int tid, uint32_t &lr0, double &cs0, uint32_t &lr1, double &cs1) {
  const int64_t e0 = e_off;
  if (tid < ne) {
    lr0 = RDY_LD(lane_ptr(a.e_lr + e0, lane_bytes(tid, 2)));
    cs0 = RDY_LD(lane_ptr(a.e_cs + e0, lane_bytes(tid, 3)));
  }
  if (tid + TILE < ne) {
    lr1 = RDY_LD(lane_ptr(a.e_lr + (e0 + TILE), lane_bytes(tid, 2)));
    cs1 = RDY_LD(lane_ptr(a.e_cs + (e0 + TILE), lane_bytes(tid, 3)));
  }
}
// ... of the table kernels: the words alone, a record's normal is entry (word >> EDGE_NT_SHIFT) of the LDS table
__device__ __forceinline__ void load_record_words(const KernelArgs &a, int e_off, int ne, int tid, uint32_t &lr0, uint32_t &lr1) {
  const int64_t e0 = e_off;
  if (tid < ne) lr0 = RDY_LD(lane_ptr(a.e_lr + e0, lane_bytes(tid, 2)));
  if (tid + TILE < ne) lr1 = RDY_LD(lane_ptr(a.e_lr + (e0 + TILE), lane_bytes(tid, 2)));
}

// Persistent, software-pipelined form: a workgroup walks a sequence of tiles.
// All index and geometry data is static and u is read-only during the launch,
// so every global load of tile T+1 is issued while tile T is being computed
// (and the halo-cell ids of T+2 as well): its cell states and edge records
// after T's first barrier, its per-cell streams at the end of T, into the
// registers T's phase 2 has just read for the last time.  A tile never waits
// for a dependent chain of global loads.  The states and records have a flux
// phase to complete, the streams the store phase, phase 0 and the flux phase
// of the next tile -- only phase 2 reads them, each lane its own, so ONE
// generation of them is enough, and the registers of the second one are what
// lets a family run four workgroups per CU (tiled_blocks_per_cu).
//
// HR = hydrostatic reconstruction (ApplyInteriorFluxHR, src/swe/swe_petsc.c:1000-1161):
// each interior edge's two depths are reconstructed against max(zc_l, zc_r) before
// the Roe solver, a pressure correction 0.5 g (h^2 - h_rec^2) (cn, sn) is added per
// side, and the source term drops the bed slope (CreatePetscSWESourceHROperator, 1229-1263).
//
// EULER = the forward-Euler update fused into the store phase (what TSEULER's VecAXPY does after the RHS,
// rdyhip_euler_step): the owned rows of a second state array receive u + dt F, F itself is stored only if f != nullptr.
// The LDS planes have COMPILE-TIME lengths (side-data slots: TILE own + the tile's halo cells; edge slots) -- every tile is
// cut to those capacities at create -- so every plane offset is an instruction immediate instead of a register and an add.
// The lengths are not multiples of 64 doubles on purpose: hipcc
// would fuse the reads of two planes into ds_read2st64_b64, which the LDS serves at half the rate of two ds_read_b64.
// HR kernels stage the velocities with the HR operator's wet test, "h > tiny_h" (swe_petsc.c:1061-1064), instead of
// ComputeRiemannVelocities' "h < tiny_h => 0" (62): the edge phase then needs no per-edge selects.  The two rules differ only
// at h == tiny_h exactly, where the boundary edges and the primitive variables (which keep the other rule) recompute.
__device__ __forceinline__ void hr_velocity_rule(RiemannSide &s, double tiny_h) {
  const bool wet = s.h > tiny_h;
  s.u            = wet ? s.u : 0.0;
  s.v            = wet ? s.v : 0.0;
}
// The two reconstructed Riemann sides of an interior edge (swe_petsc.c:1046-1071) from the staged ones (velocities already
// under the HR operator's rule, hr_velocity_rule) and the two bed elevations.
__device__ __forceinline__ void hr_reconstruct(const RiemannSide &L, const RiemannSide &R, double zl, double zr, RiemannSide &Lr, RiemannSide &Rr) {
  const double z_max = fmax(zl, zr);
  Lr.h = fmax(0.0, (L.h + zl) - z_max);
  Rr.h = fmax(0.0, (R.h + zr) - z_max);
  Lr.u = L.u; Lr.v = L.v; Rr.u = R.u; Rr.v = R.v;
  // Only the side with the LOWER bed changes its depth; the other one keeps (h + z) - z, i.e. its own depth up to one
  // rounding of the sum, and its staged square root stands in for the root of that value (relative difference
  // <= ulp(h + z) / (4 h): ~1e-13 for 1 cm of water over a bed at 50 m).  One square root
  // per edge instead of two.  Where the reconstructed depth of that side is clamped to zero -- a negative depth
  // (a drying overshoot: its staged root is NaN) or a film thinner than ulp(z) -- the root is the reference's
  // sqrt(0) = 0, not the staged one (swe_petsc.c:1051-1053).
  // (equal beds: both sides keep their depth, both take their staged root -- the rule must not depend on which cell
  // is called left, or two edges that tie in the reference would not tie here)
  const bool   l_high = zl >= zr, r_high = zr >= zl;
  const double sx     = rdy_sqrt(l_high ? Rr.h : Lr.h);
  Lr.sqh = l_high ? (Lr.h > 0.0 ? L.sqh : 0.0) : sx;
  Rr.sqh = r_high ? (Rr.h > 0.0 ? R.sqh : 0.0) : sx;
  Lr.c   = SQRT_GRAVITY * Lr.sqh;
  Rr.c   = SQRT_GRAVITY * Rr.sqh;
}
// The extra Courant edges (ColdArgs::x_*), first order / HR: the largest wave speed of each, from global memory, through the
// SAME device functions as the edge phase (riemann_side, hr_reconstruct, roe_flux: every operation that feeds amax is an
// explicit fma / uncontracted product, so the value has the bits the edge phase would give it -- a tie stays a tie).  Spread
// over the threads of the launch, after its tile loop; a launch of the INTERIOR phase (no ghost data yet) skips it.
template <bool HR>
__device__ __forceinline__ void courant_extra_edges(const KernelArgs &a, double dt, const double *__restrict__ u, CourantTrack &t) {
  const int nx = RDY_COLD(a, n_xedges);
  if (nx == 0 || a.phase == RDYHIP_PHASE_INTERIOR) return;  // uniform
  const int32_t  *xlr = RDY_COLD(a, x_lr);
  const uint32_t *xfl = RDY_COLD(a, x_flags);
  const double   *xcs = RDY_COLD(a, x_cs), *xcf = RDY_COLD(a, x_cfac);
  const int       rec0 = RDY_COLD(a, x_rec0);
  for (int i = blockIdx.x * TILE + threadIdx.x; i < nx; i += gridDim.x * TILE) {
    const int64_t l = xlr[2 * i], r = xlr[2 * i + 1];
    RiemannSide   L = riemann_side(u[3 * l + 0], u[3 * l + 1], u[3 * l + 2], a.tiny_h, a.h_anuga_sq);
    RiemannSide   R = riemann_side(u[3 * r + 0], u[3 * r + 1], u[3 * r + 2], a.tiny_h, a.h_anuga_sq);
    double        cn, sn;
    edge_normal(xfl[i], xcs[i], cn, sn);
    double am;
    bool   wet = !(R.h < a.tiny_h && L.h < a.tiny_h);
    if (!HR) {
      am = roe_flux(L, R, sn, cn).amax;
    } else {
      hr_velocity_rule(L, a.tiny_h);
      hr_velocity_rule(R, a.tiny_h);
      RiemannSide Lr, Rr;
      hr_reconstruct(L, R, a.zc_local[l], a.zc_local[r], Lr, Rr);
      am  = roe_flux(Lr, Rr, sn, cn).amax;
      wet = wet && (Lr.h > a.tiny_h || Rr.h > a.tiny_h);
    }
    if (wet) {
      const double cnum = am * xcf[i] * dt;
      if (cnum > t.best) {
        t.best = cnum;
        t.rec  = rec0 + i;
        t.pos  = -1;
      } else if (cnum == t.best) {
        courant_resolve_tie(a, t, rec0 + i, 0);
      }
    }
  }
}

// Workgroups per CU (= waves per SIMD: a workgroup is one wave on each of the four SIMDs) of a (S, SRC, HR) family.  The
// persistent grid is sized once per operator and every call form runs on it, so all six OVW / EULER / FNT instantiations
// of a family share the setting.  Four needs <= 128 VGPRs and 4 x tiled_lds_bytes <= 160 KB: the HR workgroup (46 KB) cannot,
// the others are set by their own A/B timings (profiles/RESULTS_LOG.md section 15).
constexpr int tiled_blocks_per_cu(int S, int SRC, bool hr) { return (S == 3 && SRC == 0 && !hr) ? 4 : 3; }
// Whether an instantiation has the dynamic tile walk (KernelArgs::tile_walk) compiled in: the RHS / apply kernels of the family at
// four workgroups per CU, where it was measured (profiles/RESULTS_LOG.md section 21).  Not its Euler-step kernels: the draw's one
// register from the load batch to the second barrier is the 129th VGPR there (three spilled to scratch).  Not the families at
// three, whose A/B has not been run: their kernels are the code they were.  launch_rhs asks before it sets TILE_WALK_DYNAMIC.
constexpr bool tiled_has_dynamic_walk(int S, int SRC, bool hr, bool euler) { return tiled_blocks_per_cu(S, SRC, hr) == 4 && !euler; }
// FNT = false: F (EULER: u_out) is stored without the non-temporal hint (RDYHIP_CONFIG_CACHED_F_STORES / states that fit the Infinity Cache)
//
// Two kernel families share ONE body, swe_tiled_body.h, included into each below with NTAB set.  NTAB = false is
// swe_rhs_tiled_kernel: every record streams its normal (e_cs, 8 B) and rebuilds the other component (edge_normal).  NTAB = true
// is swe_rhs_ntab_kernel, for operators whose edges have at most NORMAL_TABLE_MAX distinct normals (normal_table.h): the
// workgroup runs edge_normal on the table's entries once, into LDS behind the last plane, and a record takes its (cn, sn) from
// there by the index in bits 26-31 of its word -- the same function on the same operands, so the same bits -- and e_cs is not
// read.  Nothing else differs.  One signature (hot_kernargs reads the same kernarg segment in both), one set of attributes per
// (S, SRC, HR).
//      Included, not called: as a __device__ __forceinline__ function template inlined into two __global__ wrappers the same
// text compiles to other machine code for all 48 streamed kernels (operands of commutative instructions swapped, compares
// against shifted constants: the same results, but no kernel the profiles were measured on), whether the arguments go by
// value or by reference, with or without __restrict__.  In place, the streamed kernels are byte for byte what they were.
template <int S, int SRC, bool OVW, bool HR, bool EULER = false, bool FNT = true>
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(tiled_blocks_per_cu(S, SRC, HR), tiled_blocks_per_cu(S, SRC, HR)))) void swe_rhs_tiled_kernel(const KernelArgs a, const double dt, const double *__restrict__ u,
                                                              double *__restrict__ f) {
  constexpr bool NTAB = false;
#include "swe_tiled_body.h"
}
template <int S, int SRC, bool OVW, bool HR, bool EULER = false, bool FNT = true>
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(tiled_blocks_per_cu(S, SRC, HR), tiled_blocks_per_cu(S, SRC, HR)))) void swe_rhs_ntab_kernel(const KernelArgs a, const double dt, const double *__restrict__ u,
                                                             double *__restrict__ f) {
  constexpr bool NTAB = true;
#include "swe_tiled_body.h"
}

// ---------------------------------------------------------------------------
// cell-centric kernel: one thread = one owned cell, all of its edges
// ---------------------------------------------------------------------------
// The neighbour ids of owned cell o, and whether the cell is of the launch's phase: ghost adjacency is the NBR_GHOST bit of an
// id (a.phase is uniform per launch).  For the cell-centric kernels here and in tracer_kernels.h.  (`active` as a variable,
// not early returns: with those swe_rhs_kernel compiles to other machine code.)
template <int S>
__device__ __forceinline__ bool cell_of_phase(const KernelArgs &a, const int32_t *nbr, int o, int32_t *id) {
  bool active = true, has_ghost = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    id[s] = nbr[s * a.stride + o];
    has_ghost |= (id[s] >= 0) && (id[s] & NBR_GHOST);
  }
  if (a.phase == RDYHIP_PHASE_INTERIOR && has_ghost) active = false;
  if (a.phase == RDYHIP_PHASE_HALO && !has_ghost) active = false;
  return active;
}

template <int S, int SRC>
__global__ __launch_bounds__(BLOCK) void swe_rhs_kernel(const KernelArgs a, const double dt, const double *__restrict__ u,
                                                        double *__restrict__ f) {
  const int i = xcd_block(a.xcd_chunks) * BLOCK + threadIdx.x;

  double best      = 0.0;  // largest Courant number seen by this thread (> 0 only)
  int    best_slot = -1;
  int    o         = 0;

  bool    active = i < a.n_work;
  int32_t id[S];
  const int32_t *nbr = RDY_COLD(a, nbr), *btype = RDY_COLD(a, btype);  // one thread = one cell: read once per thread
  const double  *cn_ = RDY_COLD(a, cn), *sn_ = RDY_COLD(a, sn), *bvalues = RDY_COLD(a, bvalues);
  if (active) {
    o      = a.list ? a.list[i] : i;
    active = cell_of_phase<S>(a, nbr, o, id);
  }

  if (active) {
    const int         c    = a.o2l ? a.o2l[o] : o;
    const double      h    = u[3 * (int64_t)c + 0];
    const double      hu   = u[3 * (int64_t)c + 1];
    const double      hv   = u[3 * (int64_t)c + 2];
    const RiemannSide self = riemann_side(h, hu, hv, a.tiny_h, a.h_anuga_sq);

    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    if (!a.overwrite) {
      acc0 = f[3 * (int64_t)o + 0];
      acc1 = f[3 * (int64_t)o + 1];
      acc2 = f[3 * (int64_t)o + 2];
    }

#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int32_t nid = id[s];
      if (S > 3 && nid == NBR_EMPTY) continue;
      const double cn   = cn_[s * a.stride + o];
      const double sn   = sn_[s * a.stride + o];
      const double coef = a.coef[s * a.stride + o];
      RoeFlux      fl;
      bool         wet;
      const double cfac = fabs(coef);  // len / area_self: the max over an edge's two cells is len / min(area_l, area_r)
      if (nid >= 0) {
        const int         n     = nid & NBR_MASK;
        const RiemannSide other = riemann_side(u[3 * (int64_t)n + 0], u[3 * (int64_t)n + 1], u[3 * (int64_t)n + 2], a.tiny_h, a.h_anuga_sq);
        const bool        self_left = coef < 0.0;
        RiemannSide       L, R;
        orient_sides(self, other, self_left, L, R);
        fl  = roe_flux(L, R, sn, cn);
        wet = !(R.h < a.tiny_h && L.h < a.tiny_h);
      } else {
        const int    k  = -1 - nid;
        BoundaryFlux bf = boundary_flux(btype[k], true, self, bvalues + 3 * (int64_t)k, sn, cn, a.tiny_h, a.h_anuga_sq);
        fl              = bf.flux;
        wet             = bf.wet;
        store_boundary_flux(a, k, fl, dt);
      }
      if (wet) {
        acc0 += fl.f0 * coef;
        acc1 += fl.f1 * coef;
        acc2 += fl.f2 * coef;
        const double cnum = fl.amax * cfac * dt;
        if (cnum > best) {
          best      = cnum;
          best_slot = s;
        }
      }
    }
    cell_epilogue<SRC>(a, o, dt, h, hu, hv, self.u, self.v, acc0, acc1, acc2, a.dzdx[o], a.dzdy[o], a.mannings[o], a.extsrc[3 * (int64_t)o + 0],
                       a.extsrc[3 * (int64_t)o + 1], a.extsrc[3 * (int64_t)o + 2], f);
  }
  block_courant_reduce<BLOCK>(a, best, RDY_COLD(a, pos), (best_slot < 0 ? 0 : best_slot) * a.stride + o);
}

// merges the per-workgroup buckets into the 16-byte diagnostic the host reads (rdyhip_update_diagnostics)
__global__ __launch_bounds__(1024) void courant_finalize_kernel(int nblk, const double *__restrict__ blk_max, const int32_t *__restrict__ blk_pos,
                                                               DeviceCourant *diag) {
  double m = 0.0;
  int    p = INT32_MAX;
  constexpr int U = 8;  // independent loads in flight per thread
  for (int base = threadIdx.x; base < nblk; base += 1024 * U) {
    double v[U];
    int    q[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int i = base + j * 1024;
      v[j]        = i < nblk ? blk_max[i] : 0.0;
      q[j]        = i < nblk ? blk_pos[i] : INT32_MAX;
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      if (v[j] > m || (v[j] == m && v[j] > 0.0 && q[j] < p)) {
        m = v[j];
        p = q[j];
      }
    }
  }
  __shared__ double s_max[16];
  __shared__ int    s_pos[16];
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
    for (int w = 0; w < 16; ++w) {
      if (s_max[w] > bm || (s_max[w] == bm && bm > 0.0 && s_pos[w] < bp)) {
        bm = s_max[w];
        bp = s_pos[w];
      }
    }
    diag->max_courant = bm;
    diag->pos         = bm > 0.0 ? bp : -1;
  }
}

// ResetOperatorDiagnostics (src/operator.c:772-784) on its own: clears every bucket
__global__ void courant_reset_kernel(int nblk, double *__restrict__ blk_max, int32_t *__restrict__ blk_pos) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nblk; i += gridDim.x * blockDim.x) {
    blk_max[i] = 0.0;
    blk_pos[i] = -1;
  }
}

// boundary edges whose left cell is a ghost: the reference still evaluates
// their Riemann problem into boundary_fluxes[b] (swe_petsc.c:574) although
// nothing is accumulated into F (588).  Diagnostic output only.
__global__ void boundary_ghost_kernel(int n, const int32_t *__restrict__ klist, const int32_t *__restrict__ bleft, const int32_t *__restrict__ btype,
                                      const double *__restrict__ bcn, const double *__restrict__ bsn, const double *__restrict__ bvalues,
                                      double *__restrict__ bflux, double *__restrict__ baccum, const double *__restrict__ u, double dt, double tiny_h,
                                      double h_anuga_sq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int         k = klist[i];
  const int         c = bleft[k];
  const RiemannSide L = riemann_side(u[3 * (int64_t)c + 0], u[3 * (int64_t)c + 1], u[3 * (int64_t)c + 2], tiny_h, h_anuga_sq);
  BoundaryFlux      bf = boundary_flux(btype[k], false, L, bvalues + 3 * (int64_t)k, bsn[k], bcn[k], tiny_h, h_anuga_sq);
  bflux[3 * (int64_t)k + 0] = bf.flux.f0;
  bflux[3 * (int64_t)k + 1] = bf.flux.f1;
  bflux[3 * (int64_t)k + 2] = bf.flux.f2;
  baccum[3 * (int64_t)k + 0] += dt * bf.flux.f0;
  baccum[3 * (int64_t)k + 1] += dt * bf.flux.f1;
  baccum[3 * (int64_t)k + 2] += dt * bf.flux.f2;
}

__global__ void pack_cells_kernel(int n, const double *__restrict__ u, const int32_t *__restrict__ ids, double *__restrict__ buf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * (int64_t)n) return;
  const int cell = (int)(i / 3), comp = (int)(i - 3 * (int64_t)cell);
  buf[i]         = u[3 * (int64_t)ids[cell] + comp];
}
__global__ void unpack_cells_kernel(int n, double *__restrict__ u, const int32_t *__restrict__ ids, const double *__restrict__ buf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * (int64_t)n) return;
  const int cell = (int)(i / 3), comp = (int)(i - 3 * (int64_t)cell);
  u[3 * (int64_t)ids[cell] + comp] = buf[i];
}
__global__ void pack_rows_kernel(int n, int ncomp, const double *__restrict__ src, const int32_t *__restrict__ ids, double *__restrict__ buf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * ncomp) return;
  const int row = (int)(i / ncomp), comp = (int)(i - (int64_t)row * ncomp);
  buf[i]        = src[(int64_t)ids[row] * ncomp + comp];
}
__global__ void unpack_rows_kernel(int n, int ncomp, double *__restrict__ dst, const int32_t *__restrict__ ids, const double *__restrict__ buf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * ncomp) return;
  const int row = (int)(i / ncomp), comp = (int)(i - (int64_t)row * ncomp);
  dst[(int64_t)ids[row] * ncomp + comp] = buf[i];
}
__global__ void axpy_owned_kernel(int n_owned, const int32_t *__restrict__ o2l, double dt, const double *__restrict__ f, double *__restrict__ u) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * (int64_t)n_owned) return;
  if (o2l) {
    const int o = (int)(i / 3), comp = (int)(i - 3 * (int64_t)o);
    u[3 * (int64_t)o2l[o] + comp] += dt * f[i];
  } else {
    u[i] += dt * f[i];
  }
}
// u_local[owned cell o] = u_global[o]: the local part of DMGlobalToLocal (src/rdysetup.c:1133-1134)
__global__ void copy_owned_rows_kernel(int n_owned, const int32_t *__restrict__ o2l, const double *__restrict__ u_global, double *__restrict__ u_local) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * (int64_t)n_owned) return;
  const int o = (int)(i / 3), comp = (int)(i - 3 * (int64_t)o);
  u_local[3 * (int64_t)o2l[o] + comp] = u_global[i];
}
// u_out[owned cell o] = u_in[o] + dt * f[o]  (fallback of rdyhip_euler_step for the kernels without the fused update)
__global__ void euler_out_kernel(int n_owned, const int32_t *__restrict__ o2l, double dt, const double *__restrict__ f, const double *__restrict__ u_in,
                                 double *__restrict__ u_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * (int64_t)n_owned) return;
  int64_t j = i;
  if (o2l) {
    const int o = (int)(i / 3), comp = (int)(i - 3 * (int64_t)o);
    j           = 3 * (int64_t)o2l[o] + comp;
  }
  u_out[j] = u_in[j] + dt * f[i];
}
// pv[owned cell o] = (h, u, v) of u[o]: the primitive variables that the RHS kernels store once somebody has asked for them
// (KernelArgs::pv), for the first request after evaluations that did not.  The same riemann_side as theirs: the same bits.
__global__ void primitive_variables_kernel(int n_owned, const int32_t *__restrict__ o2l, double tiny_h, double h_anuga_sq, const double *__restrict__ u,
                                           double *__restrict__ pv) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_owned) return;
  const int64_t     c = o2l ? o2l[o] : o;
  const RiemannSide s = riemann_side(u[3 * c + 0], u[3 * c + 1], u[3 * c + 2], tiny_h, h_anuga_sq);
  pv[3 * o + 0]       = s.h;
  pv[3 * o + 1]       = s.u;
  pv[3 * o + 2]       = s.v;
}
__global__ void scatter_component_kernel(int n, const int32_t *__restrict__ ids, const double *__restrict__ vals, double *__restrict__ dst, int ncomp,
                                         int comp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int o                    = ids ? ids[i] : i;
  dst[(int64_t)o * ncomp + comp] = vals[i];
}

}  // namespace rdyhip
