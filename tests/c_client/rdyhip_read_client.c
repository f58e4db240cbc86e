/* RDyAdvance + RDyGetOwnedCell{Heights,XMomenta,YMomenta} in plain C11 on the native operator: fused Euler steps at a fixed dt as
 * rdyhip_advance_client.c runs them, and after every interval the three owned-cell planes through the non-blocking read-out --
 * rdyhip_state_read_begin behind the interval's last step, the NEXT interval's steps enqueued, and only then
 * rdyhip_state_read_wait + rdyhip_state_read_get (the third plane through rdyhip_state_read_ptr).  The device is never
 * drained inside the loop.  At the end rdyhip_error_sums of the final state against zeros (l1[0] = the water volume).
 *
 *   rdyhip_read_client case.bin out.bin num_intervals interval_seconds dt
 *
 * Writes to out.bin: int32 num_intervals, int32 num_owned_cells, then per interval the planes h, hu, hv [3][num_owned_cells],
 * then the RDyHipErrorSums (10 doubles).  tests/test_gpu_read_client.py compares it with the Python stepper, bit for bit. */
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

/* the planes of the read begun last, into planes[3][no] */
static int collect(RDyHipOperator op, int32_t no, double *planes) {
  const double *hv = NULL;
  CHECK(rdyhip_state_read_wait(op));
  CHECK(rdyhip_state_read_get(op, RDYHIP_COMPONENT_H, no, planes));
  CHECK(rdyhip_state_read_get(op, RDYHIP_COMPONENT_HU, no, planes + (size_t)no));
  CHECK(rdyhip_state_read_ptr(op, RDYHIP_COMPONENT_HV, &hv));
  if (no > 0) memcpy(planes + 2 * (size_t)no, hv, sizeof(double) * (size_t)no);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 6) return 1;
  CaseFile c;
  if (case_read(argv[1], &c)) return 1;
  const int32_t num_intervals = atoi(argv[3]);
  const double  interval = atof(argv[4]), dt = atof(argv[5]);
  const int32_t nc = c.hdr[0], no = c.hdr[1], nb = c.hdr[4];
  if (num_intervals < 1 || !(interval > 0.0) || !(dt > 0.0)) return 1;

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

  const size_t plane3 = 3 * (size_t)no;
  double      *planes = malloc(sizeof(double) * (plane3 * (size_t)num_intervals + 1));
  int          cur = 0, ready_seen = 0, steps = 0;
  double       time = 0.0;
  for (int iv = 0; iv < num_intervals; ++iv) {
    const double t_end = time + interval;
    while (time < t_end * (1.0 - 1e-14)) {
      const double h = fmin(dt, t_end - time); /* TS_EXACTFINALTIME_MATCHSTEP */
      CHECK(rdyhip_euler_step(op, RDYHIP_PHASE_ALL, RDYHIP_PHASE_RESET_DIAGNOSTICS, h, d_u[cur], d_u[1 - cur], NULL, st));
      cur = 1 - cur;
      time += h;
      ++steps;
    }
    /* the interval's steps are enqueued: now the planes of the interval before it, whose state these steps have overwritten since */
    if (iv > 0) {
      int rc = collect(op, no, planes + plane3 * (size_t)(iv - 1));
      if (rc) return rc;
    }
    CHECK(rdyhip_state_read_begin(op, RDYHIP_COMPONENT_H | RDYHIP_COMPONENT_HU | RDYHIP_COMPONENT_HV, d_u[cur], st));
    int32_t ready = -1;
    CHECK(rdyhip_state_read_ready(op, &ready));
    if (ready != 0 && ready != 1) return 5;
    ready_seen += ready;
  }
  {
    int rc = collect(op, no, planes + plane3 * (size_t)(num_intervals - 1));
    if (rc) return rc;
  }
  RDyHipErrorSums sums;
  CHECK(rdyhip_error_sums(op, d_u[cur], NULL, st));
  CHECK(rdyhip_error_sums_get(op, &sums));

  FILE *f = fopen(argv[2], "wb");
  if (!f) return 1;
  fwrite(&num_intervals, sizeof(int32_t), 1, f);
  fwrite(&no, sizeof(int32_t), 1, f);
  fwrite(planes, sizeof(double), plane3 * (size_t)num_intervals, f);
  fwrite(&sums, sizeof(sums), 1, f);
  fclose(f);
  printf("intervals %d  steps %d  water volume %.17g  area %.17g  (ready at once: %d)\n", num_intervals, steps, sums.l1[0], sums.area,
         ready_seen);
  free(planes);
  CHECK(rdyhip_destroy(&op));
  HIPCHECK(hipFree(d_u[0]));
  HIPCHECK(hipFree(d_u[1]));
  HIPCHECK(hipStreamDestroy(st));
  return 0;
}
