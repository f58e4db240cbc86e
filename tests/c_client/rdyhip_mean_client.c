/* Time-averaged output from a plain C11 host (no Python, no torch, no PETSc): N fused Euler steps of a fixed dt on two
 * ping-pong state arrays, and after each of them ONE rdyhip_output_mean_accumulate for the solution, the primitive variables
 * and the sources (AccumulateOutputVar, src/xdmf_output.c:196-206) -- the host never takes the primitive-variables or the
 * source pointer, so the evaluations store no primitive variables.  At the end ComputeMean (211-230) of each variable.
 *
 *   rdyhip_mean_client case.bin out.bin num_steps dt
 *
 * Writes to out.bin: int64 number of steps taken, double accumulated time, then the three means [num_owned_cells][3] in the
 * order solution, primitive variables, sources.  tests/test_gpu_output_mean.py compares it with the same calls from Python. */
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
  const int32_t all = RDYHIP_OUTPUT_SOLUTION | RDYHIP_OUTPUT_PRIMITIVE_VARIABLES | RDYHIP_OUTPUT_SOURCES;

  RDyHipConfig   cfg = {c.scal[0], c.scal[1], c.scal[2], c.hdr[5], RDYHIP_RIEMANN_ROE};
  RDyHipOperator op  = NULL;
  CHECK(rdyhip_create(&cfg, &c.mesh, nb, c.boundaries, &op));
  hipStream_t st;
  HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  CHECK(rdyhip_set_mannings_on(op, no, NULL, c.mannings, st));
  for (int k = 0; k < 3; ++k) CHECK(rdyhip_set_external_source_on(op, k, no, NULL, c.extsrc + (size_t)k * no, st));
  for (int i = 0; i < nb; ++i) CHECK(rdyhip_set_boundary_values_on(op, i, 0, 3, c.boundaries[i].num_edges, c.bvals[i], st));

  RDyHipLayoutInfo before, after;
  CHECK(rdyhip_layout_info(op, &before));
  CHECK(rdyhip_output_mean_enable(op, all));
  CHECK(rdyhip_layout_info(op, &after));
  if (after.device_bytes - before.device_bytes != 3 * 24 * (int64_t)no) {
    fprintf(stderr, "accumulators: device_bytes grew by %lld\n", (long long)(after.device_bytes - before.device_bytes));
    return 5;
  }

  const size_t bytes = sizeof(double) * 3 * (size_t)nc, obytes = sizeof(double) * 3 * (size_t)no;
  double      *d_u[2], *d_mean;
  HIPCHECK(hipMalloc((void **)&d_u[0], bytes));
  HIPCHECK(hipMalloc((void **)&d_u[1], bytes));
  HIPCHECK(hipMalloc((void **)&d_mean, 3 * obytes));
  HIPCHECK(hipMemcpyAsync(d_u[0], c.u, bytes, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(d_u[1], c.u, bytes, hipMemcpyHostToDevice, st)); /* keeps the ghost rows of the second array defined */

  int     cur = 0;
  int64_t steps = 0;
  for (int i = 0; i < num_steps; ++i) {
    CHECK(rdyhip_euler_step(op, RDYHIP_PHASE_ALL, RDYHIP_PHASE_RESET_DIAGNOSTICS, dt, d_u[cur], d_u[1 - cur], NULL, st));
    cur = 1 - cur;
    /* the solution: the step's output; the primitive variables: of the state the step evaluated (its input), formed in the launch */
    CHECK(rdyhip_output_mean_accumulate(op, all, dt, d_u[cur], st));
    ++steps;
  }
  int32_t stored = 1, water_only = -1;
  CHECK(rdyhip_primitive_variables_stored(op, &stored));
  CHECK(rdyhip_source_is_water_only(op, &water_only));
  if (stored) {
    fprintf(stderr, "the evaluations store primitive variables although nobody asked\n");
    return 5;
  }
  double T[3] = {0.0, 0.0, 0.0};
  for (int v = 0; v < 3; ++v) CHECK(rdyhip_output_mean_get(op, 1 << v, d_mean + (size_t)v * 3 * no, &T[v], st));
  if (T[0] != T[1] || T[1] != T[2]) return 5;
  CHECK(rdyhip_output_mean_reset(op, all, st));
  double t_after = -1.0;
  CHECK(rdyhip_output_mean_time(op, RDYHIP_OUTPUT_SOURCES, &t_after));
  if (t_after != 0.0) return 5;

  double *mean = malloc(3 * obytes + 8);
  if (!mean) return 4;
  HIPCHECK(hipMemcpyAsync(mean, d_mean, 3 * obytes, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  FILE *f = fopen(argv[2], "wb");
  if (!f) return 1;
  fwrite(&steps, sizeof(steps), 1, f);
  fwrite(&T[0], sizeof(double), 1, f);
  fwrite(mean, 1, 3 * obytes, f);
  fclose(f);
  printf("steps %lld  accumulated time %.17g  water-only source %d\n", (long long)steps, T[0], (int)water_only);
  CHECK(rdyhip_destroy(&op));
  HIPCHECK(hipFree(d_u[0]));
  HIPCHECK(hipFree(d_u[1]));
  HIPCHECK(hipFree(d_mean));
  HIPCHECK(hipStreamDestroy(st));
  free(mean);
  return 0;
}
