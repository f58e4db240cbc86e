/* rdyhip_advance_client.c's loop with the Courant read-back in two halves (rdyhip_diagnostics_begin / _wait) and a water source
 * that may change every interval: what a host with adaptive time stepping does to prepare interval k + 1 -- RDyApplyForcing
 * takes the time only (src/rdyadvance.c:351) -- while the device still finishes interval k.
 *
 *   rdyhip_pipeline_client case.bin out.bin num_intervals interval_seconds dt adaptive target_courant max_increase pipelined vary_rain
 *
 * vary_rain = 1: every interval sets the water source to component 0 of the case times 1 + 0.5 * (interval % 3), from a host
 *   array through rdyhip_set_external_source_on.
 * pipelined = 0: the reference's order -- the dt rule, the source, the steps, rdyhip_update_diagnostics + get.
 * pipelined = 1: stage the source, wait + get if a read is out, the dt rule, the steps, rdyhip_diagnostics_begin.
 * Both give the same dt sequence and the same bits.  The output is rdyhip_advance_client's: int64 number of steps taken, double
 * final dt, double final time, then the final state [num_cells][3]. */
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

int main(int argc, char **argv) {
  if (argc < 11) return 1;
  CaseFile c;
  if (case_read(argv[1], &c)) return 1;
  const int    num_intervals = atoi(argv[3]);
  const double interval      = atof(argv[4]);
  double       dt            = atof(argv[5]);
  const int    adaptive      = atoi(argv[6]);
  const double target        = atof(argv[7]);
  const double max_increase  = atof(argv[8]);
  const int    pipelined     = atoi(argv[9]);
  const int    vary_rain     = atoi(argv[10]);
  const int32_t nc = c.hdr[0], no = c.hdr[1], nb = c.hdr[4];

  RDyHipConfig   cfg = {c.scal[0], c.scal[1], c.scal[2], c.hdr[5], RDYHIP_RIEMANN_ROE};
  RDyHipOperator op  = NULL;
  CHECK(rdyhip_create(&cfg, &c.mesh, nb, c.boundaries, &op));
  hipStream_t st;
  HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  CHECK(rdyhip_set_mannings_on(op, no, NULL, c.mannings, st));
  for (int k = 0; k < 3; ++k) CHECK(rdyhip_set_external_source_on(op, k, no, NULL, c.extsrc + (size_t)k * no, st));
  for (int i = 0; i < nb; ++i) CHECK(rdyhip_set_boundary_values_on(op, i, 0, 3, c.boundaries[i].num_edges, c.bvals[i], st));

  const size_t bytes = sizeof(double) * 3 * (size_t)nc;
  double      *d_u[2];
  HIPCHECK(hipMalloc((void **)&d_u[0], bytes));
  HIPCHECK(hipMalloc((void **)&d_u[1], bytes));
  HIPCHECK(hipMemcpyAsync(d_u[0], c.u, bytes, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(d_u[1], c.u, bytes, hipMemcpyHostToDevice, st));
  double *rain = malloc(sizeof(double) * (size_t)(no > 0 ? no : 1));
  if (!rain) return 1;

  int     cur = 0, read_out = 0;
  int64_t steps = 0;
  double  time = 0.0, max_courant = -1.0; /* < 0: diagnostics not valid yet */
  for (int iv = 0; iv < num_intervals; ++iv) {
    if (vary_rain) {
      const double scale = 1.0 + 0.5 * (double)(iv % 3);
      for (int32_t o = 0; o < no; ++o) rain[o] = c.extsrc[o] * scale;
    }
    if (pipelined) {
      /* the source is staged while the device may still be running the last interval's steps; the setter copies `rain` */
      if (vary_rain) CHECK(rdyhip_set_external_source_on(op, 0, no, NULL, rain, st));
      if (read_out) {
        RDyHipCourant cd;
        CHECK(rdyhip_diagnostics_wait(op, RDYHIP_DIAGNOSTICS_OPERATOR));
        CHECK(rdyhip_get_diagnostics(op, &cd));
        max_courant = cd.max_courant_num;
        read_out    = 0;
      }
    }
    if (adaptive && max_courant >= 0.0) { /* src/rdyadvance.c:308-330 */
      if (max_courant < target) {
        const double ratio = max_courant > 0.0 ? target / max_courant : INFINITY;
        dt *= fmin(ratio, max_increase);
        dt = fmin(dt, interval);
      } else {
        dt *= target / max_courant;
      }
    }
    if (!pipelined && vary_rain) CHECK(rdyhip_set_external_source_on(op, 0, no, NULL, rain, st));
    const double t_end = time + interval;
    CHECK(rdyhip_reset_diagnostics(op, st));
    while (time < t_end * (1.0 - 1e-14)) {
      const double h = fmin(dt, t_end - time); /* TS_EXACTFINALTIME_MATCHSTEP */
      CHECK(rdyhip_euler_step(op, RDYHIP_PHASE_ALL, RDYHIP_PHASE_RESET_DIAGNOSTICS, h, d_u[cur], d_u[1 - cur], NULL, st));
      cur = 1 - cur;
      time += h;
      ++steps;
    }
    if (adaptive && pipelined) {
      CHECK(rdyhip_diagnostics_begin(op, RDYHIP_DIAGNOSTICS_OPERATOR, st));
      read_out = 1;
    } else if (adaptive) {
      RDyHipCourant cd;
      CHECK(rdyhip_update_diagnostics(op, st));
      CHECK(rdyhip_get_diagnostics(op, &cd));
      max_courant = cd.max_courant_num;
    }
  }
  if (read_out) CHECK(rdyhip_diagnostics_wait(op, RDYHIP_DIAGNOSTICS_OPERATOR)); /* the end of the run collects */
  double *u_out = malloc(bytes);
  if (!u_out) return 1;
  HIPCHECK(hipMemcpyAsync(u_out, d_u[cur], bytes, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  FILE *f = fopen(argv[2], "wb");
  if (!f) return 1;
  fwrite(&steps, sizeof(steps), 1, f);
  fwrite(&dt, sizeof(dt), 1, f);
  fwrite(&time, sizeof(time), 1, f);
  fwrite(u_out, 1, bytes, f);
  fclose(f);
  printf("steps %lld  final dt %.17g  time %.17g\n", (long long)steps, dt, time);
  CHECK(rdyhip_destroy(&op));
  HIPCHECK(hipFree(d_u[0]));
  HIPCHECK(hipFree(d_u[1]));
  HIPCHECK(hipStreamDestroy(st));
  free(rain);
  free(u_out);
  return 0;
}
