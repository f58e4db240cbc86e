/* The time series of WriteTimeSeries (src/time_series.c:530-564) from a plain C11 host (no Python, no torch, no PETSc): fused
 * Euler steps on two ping-pong state arrays with the monitor's calls around them -- one before the first step and one after
 * every step: a record of the observation sites, rdyhip_series_boundary_fluxes_add_time, a boundary-flux record -- all on one
 * non-blocking stream, and ONE read of each log at the end.  Nothing between the steps synchronises.
 *
 *   rdyhip_series_client case.bin
 *
 * case.bin: a case file as tests/test_gpu_c_client.py writes it (case_io.h), followed by a trailer
 *   int32 num_steps | double dt[num_steps] | int32 num_sites | int32 sites[num_sites] | int32 num_listed (-1: all boundaries) |
 *   int32 listed[max(num_listed, 0)] | int32 E | double times[num_steps + 1] | double flux records [num_steps + 1][E][3] |
 *   double observation records [num_steps + 1][num_sites][3] | int64 length of the trailer in bytes (this word not counted)
 * The records this host keeps must be the expected ones: the same 64 bits, or a NaN where a NaN is expected. */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <string.h>

#include "case_io.h"

#define CHECK(call)                                                             \
  do {                                                                          \
    int rc_ = (call);                                                           \
    if (rc_ != 0) {                                                             \
      fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, rdyhip_last_error()); \
      return 2;                                                                 \
    }                                                                           \
  } while (0)
#define HIPCHECK(call)                                                  \
  do {                                                                  \
    hipError_t e_ = (call);                                             \
    if (e_ != hipSuccess) {                                             \
      fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_)); \
      return 3;                                                         \
    }                                                                   \
  } while (0)

/* number of entries that differ: not the same bits and not NaN on both sides */
static int64_t mismatches(const char *what, const double *got, const double *exp, size_t n) {
  int64_t bad = 0;
  for (size_t i = 0; i < n; ++i) {
    if (memcmp(&got[i], &exp[i], 8) == 0 || (isnan(got[i]) && isnan(exp[i]))) continue;
    if (!bad) fprintf(stderr, "%s: entry %zu is %.17g, expected %.17g\n", what, i, got[i], exp[i]);
    ++bad;
  }
  return bad;
}

int main(int argc, char **argv) {
  if (argc < 2) return 1;
  CaseFile c;
  if (case_read(argv[1], &c)) return 1;
  const int32_t nc = c.hdr[0], no = c.hdr[1], nb = c.hdr[4];

  /* the trailer */
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  int64_t tlen = 0;
  if (fseek(f, -8, SEEK_END) || fread(&tlen, 8, 1, f) != 1 || tlen <= 0 || fseek(f, -8 - (long)tlen, SEEK_END)) return 4;
  int32_t num_steps = 0, num_sites = 0, num_listed = 0, E_exp = 0;
  if (fread(&num_steps, 4, 1, f) != 1 || num_steps < 1) return 4;
  double *dts = case_rd(f, (size_t)num_steps, 8);
  if (fread(&num_sites, 4, 1, f) != 1 || num_sites < 0) return 4;
  int32_t *sites = case_rd(f, (size_t)num_sites, 4);
  if (fread(&num_listed, 4, 1, f) != 1) return 4;
  int32_t *listed = num_listed >= 0 ? case_rd(f, (size_t)num_listed, 4) : NULL;
  if (fread(&E_exp, 4, 1, f) != 1 || E_exp < 0) return 4;
  const int32_t nrec      = num_steps + 1;
  double       *times_exp = case_rd(f, (size_t)nrec, 8);
  double       *flux_exp  = case_rd(f, (size_t)nrec * E_exp * 3, 8);
  double       *obs_exp   = case_rd(f, (size_t)nrec * num_sites * 3, 8);
  fclose(f);

  RDyHipConfig   cfg = {c.scal[0], c.scal[1], c.scal[2], c.hdr[5], RDYHIP_RIEMANN_ROE};
  cfg.well_balancing = c.hdr[7];
  if (c.zc) c.mesh.cell_zc = c.zc;
  RDyHipOperator op = NULL;
  CHECK(rdyhip_create(&cfg, &c.mesh, nb, c.boundaries, &op));
  hipStream_t st;
  HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  CHECK(rdyhip_set_mannings_on(op, no, NULL, c.mannings, st));
  for (int k = 0; k < 3; ++k) CHECK(rdyhip_set_external_source_on(op, k, no, NULL, c.extsrc + (size_t)k * no, st));
  for (int i = 0; i < nb; ++i) CHECK(rdyhip_set_boundary_values_on(op, i, 0, 3, c.boundaries[i].num_edges, c.bvals[i], st));

  /* the plan without a device = the plan of the operator */
  int32_t  K = 0, E_plan = -1, E = -1;
  for (int i = 0; i < nb; ++i) K += c.boundaries[i].num_edges;
  int32_t *plan_edge = malloc(sizeof(int32_t) * (size_t)(K > 0 ? K : 1)), *plan_bnd = malloc(sizeof(int32_t) * (size_t)(K > 0 ? K : 1));
  if (!plan_edge || !plan_bnd) return 4;
  CHECK(rdyhip_series_plan_boundary_edges(&c.mesh, nb, c.boundaries, num_listed, listed, &E_plan, plan_edge, plan_bnd));

  RDyHipLayoutInfo before, after;
  CHECK(rdyhip_layout_info(op, &before));
  CHECK(rdyhip_series_observations_enable(op, num_sites, sites, nrec));
  CHECK(rdyhip_series_boundary_fluxes_enable(op, num_listed, listed, nrec));
  CHECK(rdyhip_layout_info(op, &after));
  const int32_t *edge = NULL, *bnd = NULL;
  CHECK(rdyhip_series_boundary_edges(op, &E, &edge, &bnd));
  if (E != E_exp || E != E_plan || (E > 0 && (memcmp(edge, plan_edge, sizeof(int32_t) * (size_t)E) || memcmp(bnd, plan_bnd, sizeof(int32_t) * (size_t)E)))) {
    fprintf(stderr, "recorded edges: operator %d, plan %d, expected %d\n", (int)E, (int)E_plan, (int)E_exp);
    return 5;
  }
  const int64_t grown = 24 * (int64_t)nrec * (E + num_sites) + 4 * (int64_t)num_sites + 12 * (int64_t)K;
  if (after.device_bytes - before.device_bytes != grown) {
    fprintf(stderr, "logs and tables: device_bytes grew by %lld, expected %lld\n", (long long)(after.device_bytes - before.device_bytes), (long long)grown);
    return 5;
  }
  /* a second enable, an unknown kind: user errors */
  if (rdyhip_series_observations_enable(op, num_sites, sites, nrec) != RDYHIP_ERR_USER || rdyhip_series_clear(op, 3) != RDYHIP_ERR_USER) return 5;

  const size_t bytes = sizeof(double) * 3 * (size_t)nc;
  double      *d_u[2];
  HIPCHECK(hipMalloc((void **)&d_u[0], bytes));
  HIPCHECK(hipMalloc((void **)&d_u[1], bytes));
  HIPCHECK(hipMemcpyAsync(d_u[0], c.u, bytes, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(d_u[1], c.u, bytes, hipMemcpyHostToDevice, st)); /* keeps the ghost rows of the second array defined */

  int    cur  = 0;
  double now  = 0.0;
  for (int step = 0; step <= num_steps; ++step) {
    if (step > 0) {
      const double dt = dts[step - 1];
      CHECK(rdyhip_euler_step(op, RDYHIP_PHASE_ALL, RDYHIP_PHASE_RESET_DIAGNOSTICS, dt, d_u[cur], d_u[1 - cur], NULL, st));
      cur = 1 - cur;
      now += dt;
    }
    /* WriteTimeSeries(ts, step, time, X), both intervals 1 */
    CHECK(rdyhip_series_record(op, RDYHIP_SERIES_OBSERVATIONS, now, d_u[cur], st));
    CHECK(rdyhip_series_boundary_fluxes_add_time(op, dts[step > 0 ? step - 1 : 0]));
    CHECK(rdyhip_series_record(op, RDYHIP_SERIES_BOUNDARY_FLUXES, now, NULL, st));
  }
  /* the logs are full now */
  if (rdyhip_series_record(op, RDYHIP_SERIES_BOUNDARY_FLUXES, now, NULL, st) != RDYHIP_ERR_USER) return 5;
  int32_t entries = -1, count = -1, capacity = -1;
  double  T       = -1.0;
  CHECK(rdyhip_series_info(op, RDYHIP_SERIES_BOUNDARY_FLUXES, &entries, &count, &capacity, &T));
  if (entries != E || count != nrec || capacity != nrec || T != 0.0) return 5;

  double *times = malloc(sizeof(double) * (size_t)nrec + 8), *flux = malloc(sizeof(double) * (size_t)nrec * E * 3 + 8),
         *obs = malloc(sizeof(double) * (size_t)nrec * num_sites * 3 + 8);
  if (!times || !flux || !obs) return 4;
  int64_t bad = 0;
  CHECK(rdyhip_series_read(op, RDYHIP_SERIES_BOUNDARY_FLUXES, 0, nrec, times, flux, st));
  bad += mismatches("flux record times", times, times_exp, (size_t)nrec);
  bad += mismatches("boundary-flux records", flux, flux_exp, (size_t)nrec * E * 3);
  CHECK(rdyhip_series_read(op, RDYHIP_SERIES_OBSERVATIONS, 0, nrec, times, obs, st));
  bad += mismatches("observation times", times, times_exp, (size_t)nrec);
  bad += mismatches("observation records", obs, obs_exp, (size_t)nrec * num_sites * 3);
  printf("%d records of %d boundary edges (%d boundary edges in all) and %d sites: %lld mismatches\n", (int)nrec, (int)E, (int)K, (int)num_sites,
         (long long)bad);
  CHECK(rdyhip_destroy(&op));
  HIPCHECK(hipFree(d_u[0]));
  HIPCHECK(hipFree(d_u[1]));
  HIPCHECK(hipStreamDestroy(st));
  free(times); free(flux); free(obs); free(plan_edge); free(plan_bnd);
  if (bad) return 6;
  printf("records ok\n");
  return 0;
}
