// Writing the operator's input fields: the boundary values, Manning n and the external source through the blocking setters
// and their stream-ordered forms (the staging ring), rdyhip_refresh_field, the water-source plane's bookkeeping and the
// device-side forcing entry points (forcing_kernels.h).  May include operator_state.h and forcing_kernels.h; included by
// rdyhip_api.hip only.
#pragma once
#include <atomic>
#include <cstring>
#include <thread>

#include "operator_state.h"
#include "forcing_kernels.h"

extern "C" {

// rdyhip_field_ptr without its side effect on the external source (the pointer does not leave the library, or leaves it const)
static int field_ptr_internal(RDyHipOperator op, RDyHipField field, double **device_ptr, int64_t *num_values) {
  if (!op || !device_ptr) return fail(RDYHIP_ERR_USER, "null argument");
  int64_t n = 0;
  switch (field) {
    case RDYHIP_FIELD_PRIMITIVE_VARIABLES: *device_ptr = op->d_pv.p; n = 3 * (int64_t)op->n_owned; break;
    case RDYHIP_FIELD_EXTERNAL_SOURCES: *device_ptr = op->d_extsrc.p; n = 3 * (int64_t)op->n_owned; break;
    case RDYHIP_FIELD_MANNINGS: *device_ptr = op->d_mannings.p; n = op->n_owned; break;
    case RDYHIP_FIELD_FLUX_DIVERGENCE:
      if (!op->keep_fdiv) return fail(RDYHIP_ERR_USER, "flux divergence is not enabled (rdyhip_enable_flux_divergence)");
      *device_ptr = op->d_fdiv.p;
      n           = 3 * (int64_t)op->n_owned;
      break;
    case RDYHIP_FIELD_GRADIENTS:
      if (!op->muscl) return fail(RDYHIP_ERR_USER, "the operator was not created with second_order");
      *device_ptr = op->d_grad.p;
      n           = 6 * (int64_t)op->n_cells;
      break;
    default: return fail(RDYHIP_ERR_USER, "unknown field %d", (int)field);
  }
  if (num_values) *num_values = n;
  return 0;
}

// The edges of boundary `boundary`, which the caller says are `num_edges`: their offset in the boundary-edge tables and their
// number (every call that names a boundary starts with this)
static int boundary_edges(RDyHipOperator op, int32_t boundary, int32_t num_edges, int32_t *off, int32_t *n) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (boundary < 0 || boundary + 1 >= (int32_t)op->h_boff.size()) return fail(RDYHIP_ERR_USER, "Invalid boundary index %d", boundary);  // operator.c CheckOperatorBoundary
  *off = op->h_boff[boundary];
  *n   = op->h_boff[boundary + 1] - *off;
  if (*n != num_edges) return fail(RDYHIP_ERR_USER, "num_edges (%d) does not match boundary.num_edges (%d)", num_edges, *n);  // operator.c:1052
  return 0;
}
// Whole rows of those edges, `ncomp` doubles each, between the host array and the device table [.][ncomp] that starts at `table`
// (the SWE, tracer or one ensemble member's boundary values or fluxes): host -> device with `to_device`, else back.  Waits for
// the device first: the evaluations run on the callers' streams (PETSc's and torch's are non-blocking), and one still in flight
// may be reading the values a setter replaces or writing the fluxes a getter reads.
static int boundary_rows_copy(RDyHipOperator op, int32_t boundary, int32_t num_edges, double *table, size_t ncomp, double *host, bool to_device) {
  int32_t off = 0, n = 0;
  int     rc  = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  if (!host) return fail(RDYHIP_ERR_USER, to_device ? "null values" : "null output");
  HIP_TRY(hipDeviceSynchronize());
  double      *rows  = table + ncomp * (size_t)off;
  const size_t bytes = sizeof(double) * ncomp * (size_t)n;
  if (to_device) HIP_TRY(hipMemcpy(rows, host, bytes, hipMemcpyHostToDevice));
  else HIP_TRY(hipMemcpy(host, rows, bytes, hipMemcpyDeviceToHost));
  return 0;
}
// ... and the components [comp_offset, comp_offset + num_comp) of `values` for them; *n = 0 where there is nothing to write
static int boundary_values_args(RDyHipOperator op, int32_t boundary, int32_t comp_offset, int32_t num_comp, int32_t num_edges, const double *values,
                                int32_t *off, int32_t *n) {
  int rc = boundary_edges(op, boundary, num_edges, off, n);
  if (rc) return rc;
  if (comp_offset < 0 || num_comp < 0 || comp_offset + num_comp > 3) return fail(RDYHIP_ERR_USER, "bad component range [%d,%d)", comp_offset, comp_offset + num_comp);
  if (num_comp == 0) *n = 0;
  if (*n > 0 && !values) return fail(RDYHIP_ERR_USER, "null values");
  return 0;
}

int rdyhip_set_boundary_values(RDyHipOperator op, int32_t boundary, int32_t comp_offset, int32_t num_comp, int32_t num_edges, const double *values) {
  if (op && comp_offset == 0 && num_comp == 3) return boundary_rows_copy(op, boundary, num_edges, op->d_bvalues.p, 3, const_cast<double *>(values), true);
  int32_t off = 0, n = 0;
  int     rc  = boundary_values_args(op, boundary, comp_offset, num_comp, num_edges, values, &off, &n);
  if (rc || n == 0) return rc;
  HIP_TRY(hipDeviceSynchronize());   // as boundary_rows_copy
  HIP_TRY(hipMemcpy2D(op->d_bvalues.p + 3 * (size_t)off + comp_offset, 3 * sizeof(double), values, num_comp * sizeof(double), num_comp * sizeof(double), n,
                      hipMemcpyHostToDevice));
  return 0;
}

// the arguments of both scatter forms: `n` values (and owned cell ids, or none: cells 0 .. n - 1); n == 0: nothing to do
static int check_scatter_args(RDyHipOperator op, int32_t n, const int32_t *ids, const double *values) {
  if (n < 0 || n > op->n_owned) return fail(RDYHIP_ERR_ARG_SIZ, "n (%d) exceeds the number of owned cells (%d)", n, op->n_owned);
  if (n == 0) return 0;
  if (!values) return fail(RDYHIP_ERR_USER, "null values");
  if (ids) {
    for (int32_t i = 0; i < n; ++i)
      if (ids[i] < 0 || ids[i] >= op->n_owned) return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "owned cell id %d out of range", ids[i]);
  }
  return 0;
}

// ---- uniform fields (uniform_fields.h) ----------------------------------------------------------------------------------
static int forcing_grid(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 2048); }
// A host write of `n` checked values into the field `uf` tracks (nullptr: a field without a mode).  Returns true where the
// write covers every owned cell with ONE value and the mode holds: the caller then uploads nothing and fills on the device
// (the same bits), so the scan of a uniform array is paid for by the copy it saves.
static bool note_host_write(RDyHipOperator op, UniformField *uf, int32_t n, const int32_t *ids, const double *values) {
  if (!uf) return false;
  if (ids || n != op->n_owned) {
    uf->write_partial(values, n);
    return false;
  }
  uf->write_whole(values, n);
  return uf->uniform;
}
static int fill_component(double *dst, int ncomp, int comp, int32_t n, double value, double *mirror, hipStream_t st) {
  hipLaunchKernelGGL(forcing_fill_kernel, dim3(forcing_grid(n)), dim3(256), 0, st, n, (const int32_t *)nullptr, value, dst, ncomp, comp);
  HIP_TRY(hipGetLastError());
  if (mirror) {
    hipLaunchKernelGGL(forcing_fill_kernel, dim3(forcing_grid(n)), dim3(256), 0, st, n, (const int32_t *)nullptr, value, mirror, 1, 0);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// `mirror`: a second destination [n_owned] that receives the same staged values (the water-source plane), or nullptr
static int scatter_component(RDyHipOperator op, double *dst, int ncomp, int comp, int32_t n, const int32_t *ids, const double *values,
                             double *mirror = nullptr, UniformField *uf = nullptr) {
  int rc = check_scatter_args(op, n, ids, values);
  if (rc || n == 0) return rc;
  HIP_TRY(hipDeviceSynchronize());  // an RHS in flight on a non-blocking stream may still read the array (and the staging buffers)
  if (note_host_write(op, uf, n, ids, values)) {
    rc = fill_component(dst, ncomp, comp, n, values[0], mirror, 0);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return 0;
  }
  rc = op->d_stage_vals.reserve((size_t)n);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(op->d_stage_vals.p, values, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  const int32_t *dids = nullptr;
  if (ids) {
    rc = op->d_stage_ids.reserve((size_t)n);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(op->d_stage_ids.p, ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    dids = op->d_stage_ids.p;
  }
  hipLaunchKernelGGL(scatter_component_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, dids, op->d_stage_vals.p, dst, ncomp, comp);
  HIP_TRY(hipGetLastError());
  if (mirror) {
    hipLaunchKernelGGL(scatter_component_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, dids, op->d_stage_vals.p, mirror, 1, 0);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

// ---- the water-source plane (RDyHipOperator_s::d_src_water) -----------------------------------------------------------
// +0.0 and nothing else: -0.0 and NaN count as a momentum source
static bool is_plus_zero(double v) {
  uint64_t bits;
  memcpy(&bits, &v, sizeof(bits));
  return bits == 0;
}
static bool all_plus_zero(const double *v, int64_t n, int64_t step = 1) {
  for (int64_t i = 0; i < n; ++i)
    if (!is_plus_zero(v[i * step])) return false;
  return true;
}
// A host-side writer of source component `comp` (arguments already checked by the caller's scatter): momentum values other
// than +0.0 end the water-only mode (no data moves: d_extsrc is always current).  Returns the plane if this write has to go
// into it as well, else nullptr.
static double *source_mirror(RDyHipOperator op, int comp, int32_t n, const double *values) {
  if (comp == 0) return op->src_water_only ? op->d_src_water.p : nullptr;
  if (op->src_water_only && n > 0 && n <= op->n_owned && values && !all_plus_zero(values, n)) op->src_water_only = false;
  return nullptr;
}

int rdyhip_set_external_source(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *owned_cell_ids, const double *values) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (comp < 0 || comp > 2) return fail(RDYHIP_ERR_USER, "bad source component %d", comp);
  return scatter_component(op, op->d_extsrc.p, 3, comp, n, owned_cell_ids, values, source_mirror(op, comp, n, values),
                           comp == 0 ? &op->uniform.source : nullptr);
}

int rdyhip_set_mannings(RDyHipOperator op, int32_t n, const int32_t *owned_cell_ids, const double *values) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  return scatter_component(op, op->d_mannings.p, 1, 0, n, owned_cell_ids, values, nullptr, &op->uniform.mannings);
}

// ---- the stream-ordered forms: no device-wide synchronisation, no blocking copy ---------------------------------------
// A slot of the staging ring with room for `bytes`, free to be written by the host (the work that read it last is through).
static int stage_acquire(RDyHipOperator op, size_t bytes, StageRing::Slot **out) {
  StageRing &r = op->stage;
  if (!r.copy) HIP_TRY(hipStreamCreateWithFlags(&r.copy, hipStreamNonBlocking));
  StageRing::Slot &s = r.slot[r.next];
  r.next = (r.next + 1) % StageRing::N;
  if (!s.copied) {
    HIP_TRY(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  }
  if (s.used) HIP_TRY(hipEventSynchronize(s.done));
  s.used = false;
  if (s.cap < bytes) {
    if (s.h) HIP_TRY(hipHostFree(s.h));
    if (s.d) HIP_TRY(hipFree(s.d));
    s.h = s.d = nullptr;
    s.cap = 0;
    const size_t cap = std::max<size_t>(bytes + bytes / 4, 4096);
    HIP_TRY(hipHostMalloc(&s.h, cap, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&s.d, cap));
    s.cap = cap;
  }
  *out = &s;
  return 0;
}
// host -> pinned -> device, `bytes` from `src` to offset `off` of the slot.  Large arrays go in 8-MB chunks through a few
// threads (one core copies ~10 GB/s: 8 B per cell take it as long as 25 RHS evaluations of that many cells), and the upload of
// a chunk starts as soon as it sits in pinned memory, beside the host copies of the chunks behind it: a caller that has just
// read the Courant struct back (adaptive dt: the device is idle) waits for max(host copy, DMA), not for their sum.
static int stage_push(RDyHipOperator op, StageRing::Slot *s, size_t off, const void *src, size_t bytes) {
  constexpr size_t CHUNK = 8u << 20;
  char            *h = (char *)s->h + off, *d = (char *)s->d + off;
  const size_t     nchunks = (bytes + CHUNK - 1) / CHUNK;
  const int        nt = (int)std::min<size_t>(4, nchunks);
  if (nt <= 1) {
    memcpy(h, src, bytes);
    HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, op->stage.copy));
    return 0;
  }
  std::vector<std::atomic<int>> ready(nchunks);
  for (auto &r : ready) r.store(0, std::memory_order_relaxed);
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([=, &ready] {
      for (size_t c = (size_t)t; c < nchunks; c += (size_t)nt) {
        const size_t o = c * CHUNK, len = std::min(CHUNK, bytes - o);
        memcpy(h + o, (const char *)src + o, len);
        ready[c].store(1, std::memory_order_release);
      }
    });
  hipError_t err = hipSuccess;
  for (size_t c = 0; c < nchunks; ++c) {
    while (!ready[c].load(std::memory_order_acquire)) std::this_thread::yield();
    const size_t o = c * CHUNK, len = std::min(CHUNK, bytes - o);
    if (err == hipSuccess) err = hipMemcpyAsync(d + o, h + o, len, hipMemcpyHostToDevice, op->stage.copy);
  }
  for (auto &t : th) t.join();
  HIP_TRY(err);
  return 0;
}
// everything pushed into the slot is on its way: `st` waits for the last upload
static int stage_ready(RDyHipOperator op, StageRing::Slot *s, hipStream_t st) {
  HIP_TRY(hipEventRecord(s->copied, op->stage.copy));
  HIP_TRY(hipStreamWaitEvent(st, s->copied, 0));
  return 0;
}
static int stage_release(StageRing::Slot *s, hipStream_t st) {
  HIP_TRY(hipEventRecord(s->done, st));
  s->used = true;
  return 0;
}

static int scatter_component_on(RDyHipOperator op, double *dst, int ncomp, int comp, int32_t n, const int32_t *ids, const double *values, hipStream_t st,
                                double *mirror = nullptr, UniformField *uf = nullptr) {
  int rc = check_scatter_args(op, n, ids, values);
  if (rc || n == 0) return rc;
  if (note_host_write(op, uf, n, ids, values)) return fill_component(dst, ncomp, comp, n, values[0], mirror, st);
  const size_t vbytes = sizeof(double) * (size_t)n, ibytes = ids ? sizeof(int32_t) * (size_t)n : 0;
  StageRing::Slot *s;
  rc = stage_acquire(op, vbytes + ibytes, &s);
  if (rc) return rc;
  rc = stage_push(op, s, 0, values, vbytes);
  if (!rc && ids) rc = stage_push(op, s, vbytes, ids, ibytes);
  if (!rc) rc = stage_ready(op, s, st);
  if (rc) return rc;
  const int32_t *dids = ids ? (const int32_t *)((const char *)s->d + vbytes) : nullptr;
  hipLaunchKernelGGL(scatter_component_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, dids, (const double *)s->d, dst, ncomp, comp);
  HIP_TRY(hipGetLastError());
  if (mirror) {
    hipLaunchKernelGGL(scatter_component_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, dids, (const double *)s->d, mirror, 1, 0);
    HIP_TRY(hipGetLastError());
  }
  return stage_release(s, st);
}

int rdyhip_set_external_source_on(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *owned_cell_ids, const double *values, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (comp < 0 || comp > 2) return fail(RDYHIP_ERR_USER, "bad source component %d", comp);
  return scatter_component_on(op, op->d_extsrc.p, 3, comp, n, owned_cell_ids, values, (hipStream_t)stream, source_mirror(op, comp, n, values),
                              comp == 0 ? &op->uniform.source : nullptr);
}

int rdyhip_set_mannings_on(RDyHipOperator op, int32_t n, const int32_t *owned_cell_ids, const double *values, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  return scatter_component_on(op, op->d_mannings.p, 1, 0, n, owned_cell_ids, values, (hipStream_t)stream, nullptr, &op->uniform.mannings);
}

int rdyhip_set_boundary_values_on(RDyHipOperator op, int32_t boundary, int32_t comp_offset, int32_t num_comp, int32_t num_edges, const double *values,
                                  void *stream) {
  int32_t off = 0, n = 0;
  int     rc  = boundary_values_args(op, boundary, comp_offset, num_comp, num_edges, values, &off, &n);
  if (rc || n == 0) return rc;
  hipStream_t      st = (hipStream_t)stream;
  const size_t     bytes = sizeof(double) * (size_t)num_comp * (size_t)n;
  StageRing::Slot *s;
  rc = stage_acquire(op, bytes, &s);
  if (rc) return rc;
  rc = stage_push(op, s, 0, values, bytes);
  if (!rc) rc = stage_ready(op, s, st);
  if (rc) return rc;
  double *dst = op->d_bvalues.p + 3 * (size_t)off;
  if (comp_offset == 0 && num_comp == 3) {
    HIP_TRY(hipMemcpyAsync(dst, s->d, bytes, hipMemcpyDeviceToDevice, st));
  } else {
    HIP_TRY(hipMemcpy2DAsync(dst + comp_offset, 3 * sizeof(double), s->d, num_comp * sizeof(double), num_comp * sizeof(double), n, hipMemcpyDeviceToDevice, st));
  }
  return stage_release(s, st);
}

int rdyhip_refresh_field(RDyHipOperator op, RDyHipField field, const double *values, int64_t num_values, int32_t values_on_device, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  double *dst = nullptr;
  int64_t n   = 0;
  if (field != RDYHIP_FIELD_EXTERNAL_SOURCES && field != RDYHIP_FIELD_MANNINGS)
    return fail(RDYHIP_ERR_USER, "rdyhip_refresh_field: only the operator's input fields (external sources, Manning n) can be written");
  int rc = field_ptr_internal(op, field, &dst, &n);
  if (rc) return rc;
  if (num_values != n) return fail(RDYHIP_ERR_ARG_SIZ, "%lld values for a device field of %lld", (long long)num_values, (long long)n);
  if (n == 0) return 0;
  if (!values) return fail(RDYHIP_ERR_USER, "null values");
  hipStream_t  st = (hipStream_t)stream;
  const size_t bytes = sizeof(double) * (size_t)n;
  const bool   source = field == RDYHIP_FIELD_EXTERNAL_SOURCES;
  if (values_on_device) {
    // this path must not block, so the host cannot look at the momentum entries: the kernels read the [owned][3] array from here on
    if (source) op->src_water_only = false;
    (source ? op->uniform.source : op->uniform.mannings).write_unseen();
    HIP_TRY(hipMemcpyAsync(dst, values, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
  }
  // the only way back into the water-only mode: a whole host array whose momentum entries are all +0.0
  bool plane = false;
  if (source) {
    plane = !op->src_escaped && all_plus_zero(values + 1, op->n_owned, 3) && all_plus_zero(values + 2, op->n_owned, 3);
    op->src_water_only = plane;
    op->uniform.source.write_whole(values, op->n_owned, 3);  // the water component of every row
  } else {
    op->uniform.mannings.write_whole(values, op->n_owned);
  }
  StageRing::Slot *s;
  rc = stage_acquire(op, bytes, &s);
  if (rc) return rc;
  rc = stage_push(op, s, 0, values, bytes);
  if (!rc) rc = stage_ready(op, s, st);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(dst, s->d, bytes, hipMemcpyDeviceToDevice, st));
  // the whole plane from the staged copy: component 0 of every row, 8 B wide at a source pitch of 24 B
  if (plane)
    HIP_TRY(hipMemcpy2DAsync(op->d_src_water.p, sizeof(double), s->d, 3 * sizeof(double), sizeof(double), (size_t)op->n_owned, hipMemcpyDeviceToDevice, st));
  return stage_release(s, st);
}

// ---- device-side forcing ingestion (forcing_kernels.h) -------------------------------------------------
static int forcing_source_args(RDyHipOperator op, int32_t comp, int32_t n) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (comp < 0 || comp > 2) return fail(RDYHIP_ERR_USER, "bad source component %d", comp);
  if (n < 0 || n > op->n_owned) return fail(RDYHIP_ERR_ARG_SIZ, "n (%d) exceeds the number of owned cells (%d)", n, op->n_owned);
  return 0;
}

int rdyhip_forcing_fill_source(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *d_owned_cell_ids, double value, void *stream) {
  int rc = forcing_source_args(op, comp, n);
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(forcing_fill_kernel, dim3(forcing_grid(n)), dim3(256), 0, (hipStream_t)stream, n, d_owned_cell_ids, value, op->d_extsrc.p, 3, comp);
  HIP_TRY(hipGetLastError());
  if (comp == 0) {
    // without ids the fill covers cells 0 .. n - 1, all owned cells if n says so; a device id list the host cannot read
    // counts as some of them
    if (!d_owned_cell_ids && n == op->n_owned) op->uniform.source.fill_whole(value);
    else op->uniform.source.fill_partial(value);
  }
  if (comp != 0) {
    if (!is_plus_zero(value)) op->src_water_only = false;
  } else if (op->src_water_only) {
    hipLaunchKernelGGL(forcing_fill_kernel, dim3(forcing_grid(n)), dim3(256), 0, (hipStream_t)stream, n, d_owned_cell_ids, value, op->d_src_water.p, 1, 0);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int rdyhip_forcing_gather_source(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *d_owned_cell_ids, const double *d_data,
                                 const int32_t *d_data2mesh_idx, int64_t stride, int64_t offset, double scale, void *stream) {
  int rc = forcing_source_args(op, comp, n);
  if (rc || n == 0) return rc;
  if (!d_data || !d_data2mesh_idx) return fail(RDYHIP_ERR_USER, "null dataset or map");
  if (stride < 1 || offset < 0) return fail(RDYHIP_ERR_USER, "bad stride/offset (%lld, %lld)", (long long)stride, (long long)offset);
  // the values are the device's: a momentum component ends the water-only mode without a look; the water component goes
  // into the [owned][3] array and, in that mode, into the plane as well (same kernel, same operands: the same bits)
  if (comp != 0) op->src_water_only = false;
  else op->uniform.source.write_unseen();
  double *const dsts[2] = {op->d_extsrc.p, comp == 0 && op->src_water_only ? op->d_src_water.p : nullptr};
  for (int k = 0; k < 2 && dsts[k]; ++k) {
    const int ncomp = k == 0 ? 3 : 1;
    if (scale == 1.0)
      hipLaunchKernelGGL(forcing_gather_kernel<false>, dim3(forcing_grid(n)), dim3(256), 0, (hipStream_t)stream, n, d_owned_cell_ids, d_data,
                         d_data2mesh_idx, stride, offset, scale, dsts[k], ncomp, comp);
    else
      hipLaunchKernelGGL(forcing_gather_kernel<true>, dim3(forcing_grid(n)), dim3(256), 0, (hipStream_t)stream, n, d_owned_cell_ids, d_data,
                         d_data2mesh_idx, stride, offset, scale, dsts[k], ncomp, comp);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int rdyhip_forcing_fill_boundary(RDyHipOperator op, int32_t boundary, int32_t num_edges, double h, void *stream) {
  int32_t off = 0, n = 0;
  int     rc  = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(forcing_fill_boundary_kernel, dim3(forcing_grid(3 * (int64_t)n)), dim3(256), 0, (hipStream_t)stream, n, h,
                     op->d_bvalues.p + 3 * (size_t)off);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_forcing_gather_boundary(RDyHipOperator op, int32_t boundary, int32_t num_edges, const double *d_data, const int32_t *d_data2mesh_idx,
                                   int64_t stride, int64_t offset, void *stream) {
  int32_t off = 0, n = 0;
  int     rc  = boundary_edges(op, boundary, num_edges, &off, &n);
  if (rc || n == 0) return rc;
  if (!d_data || !d_data2mesh_idx) return fail(RDYHIP_ERR_USER, "null dataset or map");
  if (stride < 3 || offset < 0) return fail(RDYHIP_ERR_USER, "bad stride/offset (%lld, %lld)", (long long)stride, (long long)offset);
  hipLaunchKernelGGL(forcing_gather_boundary_kernel, dim3(forcing_grid(3 * (int64_t)n)), dim3(256), 0, (hipStream_t)stream, n, d_data,
                     d_data2mesh_idx, stride, offset, op->d_bvalues.p + 3 * (size_t)off);
  HIP_TRY(hipGetLastError());
  return 0;
}

int rdyhip_forcing_nearest_map(int32_t n, const double *d_xc, const double *d_yc, int32_t ndata, const double *d_data_xc, const double *d_data_yc,
                               double min_dist0, int32_t *d_map, void *stream) {
  if (n < 0 || ndata < 0) return fail(RDYHIP_ERR_ARG_SIZ, "negative count");
  if (n == 0 || ndata == 0) return 0;
  if (!d_xc || !d_yc || !d_data_xc || !d_data_yc || !d_map) return fail(RDYHIP_ERR_USER, "null argument");
  hipLaunchKernelGGL(forcing_nearest_kernel, dim3((n + NN_BLOCK - 1) / NN_BLOCK), dim3(NN_BLOCK), 0, (hipStream_t)stream, n, d_xc, d_yc, ndata,
                     d_data_xc, d_data_yc, min_dist0, d_map);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
