// Time series on the device behind the C ABI (rdyhip_series_*; kernels: series_kernels.h, record plan: series_plan.h): the
// observation and boundary-flux logs of WriteTimeSeries.  Included by rdyhip_api.hip only.
#pragma once
namespace {

// null operator, unknown kind: the argument errors every call shares; *s = the series
int series_check(RDyHipOperator op, int32_t kind, Series **s) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (kind != RDYHIP_SERIES_OBSERVATIONS && kind != RDYHIP_SERIES_BOUNDARY_FLUXES)
    return fail(RDYHIP_ERR_USER, "unknown series kind %d (exactly one of RDYHIP_SERIES_OBSERVATIONS, RDYHIP_SERIES_BOUNDARY_FLUXES)", kind);
  *s = &op->series[kind == RDYHIP_SERIES_OBSERVATIONS ? 0 : 1];
  return 0;
}
int series_check_enabled(const Series *s, int32_t kind) {
  if (!s->enabled) return fail(RDYHIP_ERR_USER, "series %d is not enabled (rdyhip_series_%s_enable)", kind,
                               kind == RDYHIP_SERIES_OBSERVATIONS ? "observations" : "boundary_fluxes");
  return 0;
}

}  // namespace

extern "C" int rdyhip_series_observations_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids, int32_t capacity) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  std::vector<int32_t> local;
  int rc = series_sites(op, op->series[0], SWE_WORDS, num_sites, owned_cell_ids, capacity, local);
  if (rc) return rc;
  Series s;
  rc = s.d_sites.upload(local);
  if (!rc) rc = series_alloc_log(&s, num_sites, capacity, 3);
  if (!rc) op->series[0] = std::move(s);
  return rc;
}

extern "C" int rdyhip_series_boundary_fluxes_enable(RDyHipOperator op, int32_t num_listed, const int32_t *boundaries, int32_t capacity) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (capacity < 0) return fail(RDYHIP_ERR_USER, "negative capacity (%d)", capacity);
  const int32_t        nb = (int32_t)op->h_boff.size() - 1;
  std::vector<uint8_t> mask;
  int                  rc = series_listed_mask(nb, num_listed, boundaries, mask);
  if (rc) return rc;
  if (op->series[1].enabled) return fail(RDYHIP_ERR_USER, "the boundary-flux series is enabled already");
  std::vector<uint8_t> left_owned((size_t)op->K, 1);
  for (int32_t k : op->h_bghost) left_owned[(size_t)k] = 0;
  SeriesPlan P;
  series_plan_rows(nb, op->h_boff.data(), op->h_bedge.data(), left_owned.data(), mask, P);
  Series s;
  rc = s.d_slot.upload(P.slot);
  if (!rc) rc = s.d_len.upload(op->h_blen);
  if (!rc) rc = series_alloc_log(&s, P.E, capacity, 3);
  if (rc) return rc;
  s.h_edge = std::move(P.edge);
  s.h_bnd  = std::move(P.boundary);
  op->series[1] = std::move(s);
  return 0;
}

extern "C" int rdyhip_series_boundary_edges(RDyHipOperator op, int32_t *num_edges, const int32_t **local_edge_ids, const int32_t **boundary_of_edge) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  int rc = series_check_enabled(&op->series[1], RDYHIP_SERIES_BOUNDARY_FLUXES);
  if (rc) return rc;
  if (num_edges) *num_edges = op->series[1].entries;
  if (local_edge_ids) *local_edge_ids = op->series[1].h_edge.data();
  if (boundary_of_edge) *boundary_of_edge = op->series[1].h_bnd.data();
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
  op->series[1].btime += dt;   // AccumulateBoundaryFluxes: accumulated_time += dt
  return 0;
}

extern "C" int rdyhip_series_record(RDyHipOperator op, int32_t kind, double time, const double *u_local, void *stream) {
  Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  const bool obs = kind == RDYHIP_SERIES_OBSERVATIONS;
  if (obs && s->entries > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local (needed with RDYHIP_SERIES_OBSERVATIONS)");
  if (s->records >= s->capacity)
    return fail(RDYHIP_ERR_USER, "series %d: the log is full (%d records); read it and call rdyhip_series_clear", kind, s->capacity);
  const int64_t r = s->records;
  if (s->entries > 0) {
    if (obs) {
      hipLaunchKernelGGL(series_observe_kernel, dim3((unsigned)((s->entries + SERIES_BLOCK - 1) / SERIES_BLOCK)), dim3(SERIES_BLOCK), 0, (hipStream_t)stream,
                         s->entries, s->d_sites.p, u_local, r, s->d_log.p);
    } else {
      // WriteBoundaryFluxes (src/time_series.c:311-313): no accumulated time divides by 1
      const double T = s->btime == 0.0 ? 1.0 : s->btime;
      hipLaunchKernelGGL(series_boundary_record_kernel, dim3((unsigned)((op->K + SERIES_BLOCK - 1) / SERIES_BLOCK)), dim3(SERIES_BLOCK), 0, (hipStream_t)stream,
                         op->K, s->d_slot.p, s->d_len.p, T, r, (int64_t)s->entries, op->d_baccum.p, s->d_log.p);
    }
    HIP_TRY(hipGetLastError());
  }
  s->times.push_back(time);
  ++s->records;
  if (!obs) s->btime = 0.0;   // ResetAccumulatedBoundaryFluxes
  return 0;
}

extern "C" int rdyhip_series_info(RDyHipOperator op, int32_t kind, int32_t *entries, int32_t *count, int32_t *capacity, double *accumulated_time) {
  Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  series_info(*s, entries, count, capacity);
  if (accumulated_time) *accumulated_time = s->btime;   // the observations' stays 0
  return 0;
}

extern "C" int rdyhip_series_read(RDyHipOperator op, int32_t kind, int32_t first, int32_t count, double *times, double *values, void *stream) {
  Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  const std::string name = "series " + std::to_string(kind);
  return series_read(*s, name.c_str(), (size_t)s->entries * 3, 1, first, count, times, values, (hipStream_t)stream);
}

extern "C" int rdyhip_series_device_log(RDyHipOperator op, int32_t kind, const double **d_log) {
  Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (rc) return rc;
  if (!d_log) return fail(RDYHIP_ERR_USER, "null d_log");
  rc = series_check_enabled(s, kind);
  if (rc) return rc;
  *d_log = s->d_log.p;
  return 0;
}

extern "C" int rdyhip_series_clear(RDyHipOperator op, int32_t kind) {
  Series *s = nullptr;
  int rc = series_check(op, kind, &s);
  if (!rc) rc = series_check_enabled(s, kind);
  if (rc) return rc;
  series_clear(*s);
  return 0;
}

