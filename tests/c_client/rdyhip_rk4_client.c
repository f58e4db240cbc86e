/* `numerics.temporal: rk4` from a plain C11 host (no Python, no torch, no PETSc's TS): N classical Runge-Kutta steps of a
 * fixed dt through rdyhip_rk4_step -- four stage evaluations and the tableau's vector updates behind one call per step, the
 * stage vectors in the operator's own workspace.  One rank: no halo.
 *
 *   rdyhip_rk4_client case.bin out.bin num_steps dt
 *
 * Writes to out.bin: int64 number of steps taken, double max Courant number of the last stage, then the final state
 * [num_cells][3].  tests/test_gpu_rk4_step.py compares it with the same loop driven by the CPU oracle. */
#include <hip/hip_runtime_api.h>

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
  if (argc < 5) return 1;
  CaseFile c;
  if (case_read(argv[1], &c)) return 1;
  const int     num_steps = atoi(argv[3]);
  const double  dt        = atof(argv[4]);
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
  double      *d_u;
  HIPCHECK(hipMalloc((void **)&d_u, bytes));
  HIPCHECK(hipMemcpyAsync(d_u, c.u, bytes, hipMemcpyHostToDevice, st));

  RDyHipLayoutInfo before, after;
  CHECK(rdyhip_layout_info(op, &before));
  int64_t steps = 0;
  for (int i = 0; i < num_steps; ++i) { /* TSStep_RK, TSRK4 (src/rdysetup.c:1187-1189): the first call allocates the workspace */
    CHECK(rdyhip_rk4_step(op, NULL, dt, d_u, st));
    ++steps;
  }
  CHECK(rdyhip_layout_info(op, &after));
  if (num_steps > 0 && after.device_bytes - before.device_bytes != ((int64_t)nc + 4 * (int64_t)no) * 24) {
    fprintf(stderr, "workspace: device_bytes grew by %lld\n", (long long)(after.device_bytes - before.device_bytes));
    return 5;
  }
  RDyHipCourant cd;
  CHECK(rdyhip_update_diagnostics(op, st)); /* the last stage's Courant struct */
  CHECK(rdyhip_get_diagnostics(op, &cd));
  double *u_out = malloc(bytes);
  HIPCHECK(hipMemcpyAsync(u_out, d_u, bytes, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  FILE *f = fopen(argv[2], "wb");
  if (!f) return 1;
  fwrite(&steps, sizeof(steps), 1, f);
  fwrite(&cd.max_courant_num, sizeof(double), 1, f);
  fwrite(u_out, 1, bytes, f);
  fclose(f);
  printf("steps %lld  max Courant number of the last stage %.17g\n", (long long)steps, cd.max_courant_num);
  CHECK(rdyhip_destroy(&op));
  HIPCHECK(hipFree(d_u));
  HIPCHECK(hipStreamDestroy(st));
  free(u_out);
  return 0;
}
