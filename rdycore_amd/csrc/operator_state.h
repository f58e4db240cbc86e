// What an operator is made of: the device buffers that free themselves, the staging ring of the stream-ordered setters, one
// struct of state per feature and RDyHipOperator_s.  Includes the HIP runtime and host_layout.h (for LayoutCounts); included by rdyhip_api.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "rdyhip.h"
#include "error.h"
#include "host_layout.h"
#include "uniform_fields.h"
#include "swe_kernels.h"

using namespace rdyhip;

#define HIP_TRY(expr)                                                                                       \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) return fail(RDYHIP_ERR_LIB, "%s failed: %s", #expr, hipGetErrorString(e_));       \
  } while (0)

// A device array that frees itself.  alloc / upload / zeros on a buffer that holds memory release it first.
template <typename T>
struct DevBuf {
  T     *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  int alloc(size_t count) {
    release();
    const size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t   e     = hipMalloc((void **)&p, bytes);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(RDYHIP_ERR_MEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    n = count;
    return 0;
  }
  // room for `count` elements: grows only, and the content is not kept
  int reserve(size_t count) { return p && n >= count ? 0 : alloc(count); }
  int upload(const std::vector<T> &h) {
    int rc = alloc(h.size());
    if (rc) return rc;
    if (!h.empty()) HIP_TRY(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  int zeros(size_t count) {
    int rc = alloc(count);
    if (rc) return rc;
    HIP_TRY(hipMemset(p, 0, (count ? count : 1) * sizeof(T)));
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  size_t bytes() const { return n * sizeof(T); }
};

// Staging of the stream-ordered setters (rdyhip_set_*_on): a small ring of slots, each a pinned host buffer + a device
// buffer + an event.  The caller's array is copied into the pinned buffer before the call returns (the caller may reuse it
// at once, as with the reference's setters, which copy into a Vec); the host -> device copy then runs on the operator's own
// copy stream, beside whatever the caller's stream is executing, and only the final scatter into the operator's field is
// ordered on the caller's stream.  A slot is reused once the work that read it has finished (its event).
struct StageRing {
  static constexpr int N = 4;
  struct Slot {
    void      *h = nullptr, *d = nullptr;
    size_t     cap = 0;
    hipEvent_t copied = nullptr, done = nullptr;
    bool       used = false;
  } slot[N];
  int         next = 0;
  hipStream_t copy = nullptr;
  StageRing() = default;
  StageRing(const StageRing &) = delete;
  StageRing &operator=(const StageRing &) = delete;
  ~StageRing() { release(); }
  void release() {
    for (auto &s : slot) {
      if (s.h) (void)hipHostFree(s.h);
      if (s.d) (void)hipFree(s.d);
      if (s.copied) (void)hipEventDestroy(s.copied);
      if (s.done) (void)hipEventDestroy(s.done);
      s = Slot{};
    }
    if (copy) (void)hipStreamDestroy(copy);
    copy = nullptr;
  }
};

// The pieces the output of a state is made of -- the SWE state, the [cell][3 + NT] tracer state and the [B][cell][3] ensemble state
// each hold instances of their own, so that a read of one never disturbs a read of another.  Everything is allocated by the first
// call that needs it and grows only; a piece that owns pinned memory waits for a copy that still writes it before it frees it.

// One read of planes of a state through pinned memory (rdyhip_*state_read_*; output_shared.h)
struct PlaneRead {
  enum State { NONE, IN_FLIGHT, LANDED };
  DevBuf<double> d_planes;            // ([B])[popcount(comps)][n_owned], room for the widest mask asked for so far
  double        *h_planes = nullptr;  // pinned, as many doubles as d_planes
  size_t         h_cap = 0;
  hipEvent_t     launched = nullptr, done = nullptr;   // the de-interleave launch on the caller's stream; the copy on StageRing::copy
  State          state = NONE;
  int32_t        comps = 0;           // the mask of the last begin
  PlaneRead() = default;
  PlaneRead(const PlaneRead &) = delete;
  PlaneRead &operator=(const PlaneRead &) = delete;
  ~PlaneRead() {
    if (state == IN_FLIGHT && done) (void)hipEventSynchronize(done);   // the copy writes h_planes
    if (h_planes) (void)hipHostFree(h_planes);
    if (launched) (void)hipEventDestroy(launched);
    if (done) (void)hipEventDestroy(done);
  }
};

// The error sums of a state (rdyhip_*error_sums; output_shared.h): records of `width` doubles (SWE: 10, tracers: 3 N + 1,
// ensemble: B x 10)
struct SumsRead {
  DevBuf<double>   d_records;         // [err_wg + 1][width]: the workgroups' records, then the result
  double          *h_sums = nullptr;  // pinned, `width` doubles
  hipEvent_t       done = nullptr;
  PlaneRead::State state = PlaneRead::NONE;
  SumsRead() = default;
  SumsRead(const SumsRead &) = delete;
  SumsRead &operator=(const SumsRead &) = delete;
  ~SumsRead() {
    if (state == PlaneRead::IN_FLIGHT && done) (void)hipEventSynchronize(done);   // the copy writes h_sums
    if (h_sums) (void)hipHostFree(h_sums);
    if (done) (void)hipEventDestroy(done);
  }
};

// rdyhip_*output_mean_*: one accumulator per enabled variable (bit i of RDYHIP_OUTPUT_*), [n_owned][3] for the SWE state,
// [n_owned][N] for tracers, [B][n_owned][3] for an ensemble, and the time it spans: one per member (one where there are none)
struct OutputMeans {
  DevBuf<double>      acc[3];
  std::vector<double> time[3];
  size_t bytes() const { return acc[0].bytes() + acc[1].bytes() + acc[2].bytes(); }
};

// One device log of WriteTimeSeries: `capacity` records of `entries` rows each, and the time(s) of every record on the host
// (an ensemble: B per record)
struct SeriesLog {
  bool                enabled = false;
  int32_t             entries = 0, capacity = 0, records = 0;
  DevBuf<double>      d_log;
  DevBuf<int32_t>     d_sites;          // observations: [entries] local cell of every site
  std::vector<double> times;
  size_t bytes() const { return d_log.bytes() + d_sites.bytes(); }
};

// The read-out of the SWE state (rdyhip_state_read_*, rdyhip_error_sums; readout_kernels.h).  The area table and the workgroup
// count of the error sums serve the tracer and ensemble sums too.
struct Readout {
  PlaneRead      planes;
  SumsRead       sums;
  DevBuf<double> d_area;   // [n_owned]
  int            err_wg = 0;
  size_t bytes() const { return planes.d_planes.bytes() + d_area.bytes() + sums.d_records.bytes(); }
};

// One non-blocking read of the Courant record(s) (rdyhip_diagnostics_begin / _ready / _wait; diagnostics_calls.h), one per
// scope: the pinned record(s) the copy lands in, the event recorded behind the copy, and what resolving the ids needs as of
// begin.  Pinned memory and event are allocated by the first begin of the scope; `done` is touched only while IN_FLIGHT.
struct DiagnosticsRead {
  enum State { NONE, IN_FLIGHT, LANDED };   // NONE: never begun, or discarded by the blocking call; LANDED: waited for
  DeviceCourant *h_rec = nullptr;   // pinned: 1 record (operator scope) or RDYHIP_MAX_ENSEMBLE_MEMBERS (ensemble scope)
  hipEvent_t     done = nullptr;
  State          state = NONE;
  bool           owned_side = false;  // courant_owned_side at begin
  DiagnosticsRead() = default;
  DiagnosticsRead(const DiagnosticsRead &) = delete;
  DiagnosticsRead &operator=(const DiagnosticsRead &) = delete;
  ~DiagnosticsRead() {
    if (state == IN_FLIGHT) (void)hipEventSynchronize(done);   // the copy writes h_rec
    if (h_rec) (void)hipHostFree(h_rec);
    if (done) (void)hipEventDestroy(done);
  }
};

// The features below are allocated by their enable call (RK4: the first step) and kept until destroy.  Each is built in a
// local and moved into the operator once every allocation and copy has succeeded: a failed call leaves nothing behind.
// bytes(): the device memory held, which rdyhip_layout_info reports.

// rdyhip_rk4_step: the stage state [n_cells][3] and k1..k4 [n_owned][3]; allocated: y.p is set
struct Rk4Workspace {
  DevBuf<double> y, k[4];
  size_t bytes() const { return y.bytes() + k[0].bytes() + k[1].bytes() + k[2].bytes() + k[3].bytes(); }
};

// rdyhip_series_*: the log of the observations or of the boundary fluxes, records of entries x 3 doubles
struct Series : SeriesLog {
  DevBuf<int32_t>      d_slot;           // boundary fluxes: [K] row of boundary edge k in a record, or -1
  DevBuf<double>       d_len;            //                  [K] edge lengths
  double               btime = 0.0;      //                  boundary_fluxes.accumulated_time
  std::vector<int32_t> h_edge, h_bnd;    //                  [entries] local edge id and boundary of every recorded edge
  size_t bytes() const { return SeriesLog::bytes() + d_slot.bytes() + d_len.bytes(); }
};

// rdyhip_tracers_* (tracer_kernels.h): N = 3 + n values per row.  Boundary values and fluxes [K][N] and the tracer sources
// [n_owned][n] are allocated by rdyhip_tracers_enable, the primitive variables [n_owned][N] by the first
// rdyhip_tracers_primitive_variables, from which on every tracer evaluation stores them.
struct TracerState {
  int32_t        n = 0, riemann = 0;   // 0 tracers: not enabled
  DevBuf<double> bvalues, bflux, src, pv;
  bool           pv_wanted = false;
  bool           hr = false;           // enabled by rdyhip_tracer_hr_enable: the evaluations run tracer_hr_kernel
  size_t bytes() const { return bvalues.bytes() + bflux.bytes() + src.bytes() + pv.bytes(); }
};

// rdyhip_tracer_state_* / _error_sums / _output_mean_* / _series_* (tracer_output_kernels.h) and rdyhip_ens_state_* / ... / _stats
// (ens_output_kernels.h): the read-out, the error sums, the output means and the observation series of the [cell][N = 3 + NT]
// state and of the [B][cell][3] ensemble state.  The area table of the error sums is Readout::d_area.  Means and series are
// allocated by their enable.
struct StateOutput {
  PlaneRead   planes;
  SumsRead    sums;
  OutputMeans means;
  SeriesLog   series;
  size_t bytes() const { return planes.d_planes.bytes() + sums.d_records.bytes() + means.bytes() + series.bytes(); }
};
using TracerOutput   = StateOutput;
using EnsembleOutput = StateOutput;

// rdyhip_ensemble_* (ensemble_kernels.h): B members on this operator's mesh, all allocated by rdyhip_ensemble_enable.  The
// launch is (grid, groups) workgroups, every group walking per_group members (the last one maybe fewer).
struct EnsembleState {
  int32_t                    members = 0, groups = 0, per_group = 0;   // 0 members: not enabled
  DevBuf<double>             mannings, extsrc, bvalues, bflux;   // [B][owned], [B][owned][3], [B][K][3] x 2
  DevBuf<double>             blk_max;     // [B][ENSEMBLE_WAVES * grid] one Courant bucket per member and wave
  DevBuf<int32_t>            blk_pos;
  DevBuf<DeviceCourant>      d_courant;   // [B]
  std::vector<RDyHipCourant> courant;     // [B] what rdyhip_ensemble_update_diagnostics read last
  bool                       hr = false;  // enabled by rdyhip_ens_hr_enable: the evaluations run ensemble_hr_kernel
  size_t bytes() const {
    return mannings.bytes() + extsrc.bytes() + bvalues.bytes() + bflux.bytes() + blk_max.bytes() + blk_pos.bytes() + d_courant.bytes();
  }
};

struct RDyHipHalo_s;
// (the layout's numbers -- n_cells, n_owned, S, K, n_halo, ntiles, ... -- are the base class's, copied from HostLayout::counts)
struct RDyHipOperator_s : LayoutCounts {
  StageRing stage;
  RDyHipConfig config;
  RDyHipHalo_s *fused_halo = nullptr;  // the halo whose send lists are attached to the tile descriptors (rdyhip_halo_fuse_pack)
  std::vector<int32_t> h_l2o;          // local -> owned cell id, kept only when the owned cells are not a prefix
  int          device = 0;
  int32_t      n_internal = 0;
  int64_t      stride = 0;
  int          grid = 0, xcd_chunks = 0;        // cell kernel
  int          pgrid = 0, tiled_xcd_chunks = 0; // tiled (persistent) kernel
  int          interior_shrink = 32;            // the INTERIOR phase leaves 1/interior_shrink of the workgroup slots free (0: none)
  bool         balance_rounds = false;          // size the persistent grid so that all workgroups walk the same number of tiles
  bool         keep_fdiv = false;
  // RDYHIP_TILE_WALK: PHASE_ALL launches of the first-order / HR tiled kernels over XCD chunks let their workgroups draw
  // tiles from per-XCD counters (d_tile_draw: 8 draw counters + the exit counter, a cache line apart, zero between launches) instead of a fixed share
  int             tile_walk = -1;   // -1: by size (launch_rhs), 0 / 1: RDYHIP_TILE_WALK=static / dynamic
  DevBuf<int32_t> d_tile_draw;

  DevBuf<int32_t> d_o2l, d_nbr, d_pos, d_halo_list, d_btype, d_bleft, d_bghost_list;
  DevBuf<double>  d_cn, d_sn, d_coef, d_dzdx, d_dzdy, d_mannings, d_extsrc;
  // The water source by itself, [n_owned]: a mirror of component 0 of d_extsrc (which stays the canonical array and is always
  // current), kept by every writer of the source while src_water_only holds.  The first-order / HR tiled kernels then read
  // it instead of the 24-B rows: 8 B of HBM traffic per cell where a read of any part of a row costs all 24.
  DevBuf<double>  d_src_water;
  bool            src_water_only = true;   // every momentum source is +0.0 and the plane is current
  bool            src_escaped    = false;  // rdyhip_field_ptr handed out d_extsrc: it may be written behind our back, for good
  // Fields whose owned elements all hold one 64-bit pattern (uniform_fields.h): the first-order / HR tiled kernels read
  // element 0 of the water plane, of d_mannings or of d_dzdx / d_dzdy instead of streaming the plane.  Read when a launch is
  // enqueued, like src_water_only; RDYHIP_UNIFORM_FIELDS=0 at create keeps every mode off.
  UniformFields   uniform;
  DevBuf<double>  d_bvalues, d_bflux, d_baccum, d_bcn, d_bsn, d_pv, d_fdiv, d_blk_max;
  // The primitive variables are stored by the evaluations only once somebody can look at them (rdyhip_field_ptr, until
  // rdyhip_field_release); the first request after evaluations that did not store derives them from the state of the last one.
  bool            pv_wanted  = false;    // d_pv has been handed out: every launch stores
  bool            pv_pending = false;    // at least one evaluation since the last store did not store
  const double   *pv_u       = nullptr;  // u_local of the most recent evaluation that did not store ...
  hipStream_t     pv_stream  = nullptr;  // ... and the caller's stream it was enqueued on
  DevBuf<int32_t> d_blk_pos;
  DevBuf<DeviceCourant> d_courant;
  DevBuf<ColdArgs>      d_cold;   // the kernels' rarely read pointers (swe_kernels.h), written once at create
  int32_t n_bghost = 0;
  // tiled kernel (swe_kernels.h)
  bool             use_tiled = true;
  bool             hr = false;   // hydrostatic reconstruction
  bool             uout_cached = false;  // Euler-step kernels store u_out with the default cache policy: the state fits the Infinity Cache
  DevBuf<double>   d_zc_local;
  DevBuf<TileDesc> d_tiles;
  DevBuf<uint32_t> d_e_lr;
  // The normal table (normal_table.h): > 0 entries: d_e_lr carries their indices, ColdArgs::nt_* the entries, and every
  // first-order / HR launch runs the table family (swe_rhs_ntab_kernel) with ntab_lds_bytes of LDS.  Fixed at create.
  int32_t          ntab_entries = 0;
  size_t           ntab_lds_bytes = 0;
  DevBuf<int32_t>  d_hcells, d_tile_bk, d_tile_boff, d_halo_tiles, d_e_pos, d_x_lr;
  DevBuf<uint32_t> d_x_flags;
  DevBuf<double>   d_x_cs, d_x_cfac, d_x_mid;
  int32_t          n_xedges = 0;
  std::vector<int32_t> h_tile_c0;  // [ntiles + 1] first owned cell of each tile (the fused pack's send lists are built per tile)
  DevBuf<double>   d_e_cs;
  DevBuf<uint16_t> d_slot_ref;   // S == 4
  DevBuf<uint32_t> d_slot_ref3;  // S == 3
  // second order (muscl_kernels.h)
  DevBuf<double>   d_grad, d_e_mid, d_cxy;
  DevBuf<int32_t>  d_hcells2, d_c_off;
  DevBuf<uint16_t> d_bn_idx;
  int              pgrid_muscl = 0;

  // host copies needed to resolve the Courant position into ids
  std::vector<int32_t> h_internal_edge, h_edge_cells, h_bedge, h_boff;
  std::vector<int64_t> h_cell_gid, h_edge_gid;
  std::vector<double>  h_area;
  std::vector<uint8_t> h_owned;   // [num_cells] cells.is_owned, kept on a rank with ghost cells only
  RDyHipCourant        courant{0.0, -1, -1};
  bool                 courant_owned_side = false;   // the buckets hold a tracer evaluation's numbers (courant_from_device)
  // staging buffers for the setters
  DevBuf<double>  d_scratch_f;   // F of rdyhip_euler_step when the caller wants none and the kernel cannot skip it
  DevBuf<double>  d_stage_vals;
  DevBuf<int32_t> d_stage_ids;
  // what the record plan of the boundary-flux series (series_plan.h) and the tracers' enable need of the boundary edges,
  // kept at create beside h_bedge / h_boff
  std::vector<double>  h_blen;     // [K] edges.lengths
  std::vector<int32_t> h_bghost;   // the boundary edges whose left cell is a ghost
  std::vector<int32_t> h_btype;    // [K] condition type of every boundary edge (the tracer path refuses critical outflow)
  // The features (each a struct above, with the device bytes it holds).  `readout` is declared after `stage`: its copy stream
  // outlives these buffers.
  Rk4Workspace  rk4;
  OutputMeans   means;
  Series        series[2];   // 0: observations, 1: boundary fluxes
  Readout       readout;
  TracerState   tracers;
  TracerOutput  tracer_out;
  EnsembleState ensemble;
  EnsembleOutput ens_out;
  DiagnosticsRead diag_read[2];   // RDYHIP_DIAGNOSTICS_OPERATOR, RDYHIP_DIAGNOSTICS_ENSEMBLE

  int64_t device_bytes = 0;   // what rdyhip_create allocated; rdyhip_layout_info adds the features'
  int64_t feature_bytes() const {
    return (int64_t)(rk4.bytes() + means.bytes() + series[0].bytes() + series[1].bytes() + readout.bytes() + tracers.bytes() + tracer_out.bytes() +
                     ensemble.bytes() + ens_out.bytes());
  }
};

// The owned-to-local table the kernels take: none where the owned cells are the first n_owned local cells in order
static const int32_t *owned_to_local(const RDyHipOperator_s *op) { return op->prefix ? nullptr : op->d_o2l.p; }

// What every launcher (gradients, RHS, tracers, ensembles) passes of the operator as it is; each sets only its own work,
// fields and flags on top.  A new field of KernelArgs that all of them need goes here.
static KernelArgs kernel_args_base(const RDyHipOperator_s *op) {
  KernelArgs a{};
  a.n_owned    = op->n_owned;
  a.stride     = op->stride;
  a.o2l        = owned_to_local(op);
  a.cold       = op->d_cold.p;
  a.coef       = op->d_coef.p;
  a.dzdx       = op->d_dzdx.p;
  a.dzdy       = op->d_dzdy.p;
  a.tiny_h     = op->config.tiny_h;
  a.h_anuga_sq = op->config.h_anuga_regular * op->config.h_anuga_regular;
  a.xq_thresh  = op->config.xq2018_threshold;
  return a;
}
// ... and of a launch that evaluates F(u) for all owned cells, one thread each, in one go (tracers, ensembles)
static KernelArgs kernel_args_all_cells(const RDyHipOperator_s *op) {
  KernelArgs a = kernel_args_base(op);
  a.n_work     = op->n_owned;
  a.xcd_chunks = op->xcd_chunks;
  a.overwrite  = 1;
  a.phase      = RDYHIP_PHASE_ALL;
  return a;
}
