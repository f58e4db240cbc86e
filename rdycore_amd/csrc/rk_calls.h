// The classical Runge-Kutta step behind the C ABI (rdyhip_rk4_step; kernels: rk_kernels.h): the workspace, the stage and
// combine launches, and the step itself, whose stages are the operator's own RHS calls (with the halo's overlapped form
// where there are peers).  Included by rdyhip_api.hip only, after halo_exchange.h.
#pragma once
namespace {

// the workspace of rdyhip_rk4_step, on its first call (hipMalloc: this one call may synchronise the device)
int rk4_workspace(RDyHipOperator op) {
  if (op->rk4.y.p) return 0;
  Rk4Workspace w;
  int rc = w.y.alloc((size_t)3 * op->n_cells);
  for (auto &k : w.k)
    if (!rc) rc = k.alloc((size_t)3 * op->n_owned);
  if (!rc) op->rk4 = std::move(w);
  return rc;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// y = u0 + c k on the owned rows; with `ghost_rows`, y's other rows = u0's
int launch_rk4_stage(RDyHipOperator op, double c, const double *k, const double *u0, double *y, bool ghost_rows, hipStream_t st) {
  const int64_t n_own = 3 * (int64_t)op->n_owned, n_cells3 = 3 * (int64_t)op->n_cells;
  if (!op->prefix) {
    if (ghost_rows && n_cells3 > 0) HIP_TRY(hipMemcpyAsync(y, u0, sizeof(double) * (size_t)n_cells3, hipMemcpyDeviceToDevice, st));
    if (n_own == 0) return 0;
    hipLaunchKernelGGL((rk4_stage_kernel<false>), dim3((unsigned)((n_own + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own, n_own,
                       op->d_o2l.p, c, k, u0, y);
  } else {
    const int64_t n_all = ghost_rows ? n_cells3 : n_own;
    if (n_all == 0) return 0;
    if (aligned16(k) && aligned16(u0) && aligned16(y)) {
      const int64_t pairs = (n_all + 1) / 2;
      hipLaunchKernelGGL((rk4_stage_kernel<true>), dim3((unsigned)((pairs + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own, n_all,
                         (const int32_t *)nullptr, c, k, u0, y);
    } else {
      hipLaunchKernelGGL((rk4_stage_kernel<false>), dim3((unsigned)((n_all + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own, n_all,
                         (const int32_t *)nullptr, c, k, u0, y);
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int launch_rk4_combine(RDyHipOperator op, double dt, double *u, hipStream_t st) {
  const int64_t n_own = 3 * (int64_t)op->n_owned;
  if (n_own == 0) return 0;
  const double  c1 = (1.0 / 6.0) * dt, c2 = (1.0 / 3.0) * dt, c3 = (1.0 / 3.0) * dt, c4 = (1.0 / 6.0) * dt;
  const double *k1 = op->rk4.k[0].p, *k2 = op->rk4.k[1].p, *k3 = op->rk4.k[2].p, *k4 = op->rk4.k[3].p;
  if (op->prefix && aligned16(u) && aligned16(k1) && aligned16(k2) && aligned16(k3) && aligned16(k4)) {
    const int64_t pairs = (n_own + 1) / 2;
    hipLaunchKernelGGL((rk4_combine_kernel<true>), dim3((unsigned)((pairs + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own,
                       (const int32_t *)nullptr, c1, c2, c3, c4, k1, k2, k3, k4, u);
  } else {
    hipLaunchKernelGGL((rk4_combine_kernel<false>), dim3((unsigned)((n_own + RK_BLOCK - 1) / RK_BLOCK)), dim3(RK_BLOCK), 0, st, n_own,
                       op->prefix ? (const int32_t *)nullptr : op->d_o2l.p, c1, c2, c3, c4, k1, k2, k3, k4, u);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int rdyhip_rk4_step(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, void *stream) {
  if (!op) return fail(RDYHIP_ERR_USER, "null operator");
  if (op->n_cells > 0 && !u_local) return fail(RDYHIP_ERR_USER, "null u_local");   // (ghost rows alone are still copied and exchanged)
  if (halo && halo->op != op) return fail(RDYHIP_ERR_USER, "the halo belongs to another operator");
  hipStream_t st = (hipStream_t)stream;
  // the combine kernel writes the owned rows of u_local: a send buffer that mirrors them (rdyhip_halo_fuse_pack) is stale
  if (halo) halo_forget_packed_state(halo);
  if (op->fused_halo && op->fused_halo != halo) halo_forget_packed_state(op->fused_halo);
  int rc = rk4_workspace(op);
  if (rc) return rc;
  const bool exchange = halo && !halo->peers.empty();
  // every stage is OperatorRHSFunction with its ghost update and the FULL step's dt (TSGetTimeStep, src/rdysetup.c:1129)
  auto stage_rhs = [&](double *u, double *k) -> int {
    return exchange ? overlapped(op, halo, dt, u, k, nullptr, st) : rdyhip_rhs_function(op, dt, u, k, stream);
  };
  // the stage state's ghost rows: the stage's own exchange writes them where the halo receives every one of them; the
  // others keep u_local's values
  const bool ghost_rows = op->n_cells > op->n_owned && !(exchange && halo->recv_covers_ghosts);
  double    *y = op->rk4.y.p;
  rc = stage_rhs(u_local, op->rk4.k[0].p);
  const double a[3] = {0.5, 0.5, 1.0};
  for (int j = 1; j < 4 && !rc; ++j) {
    rc = launch_rk4_stage(op, a[j - 1] * dt, op->rk4.k[j - 1].p, u_local, y, ghost_rows, st);
    if (!rc) rc = stage_rhs(y, op->rk4.k[j].p);
  }
  if (!rc) rc = launch_rk4_combine(op, dt, u_local, st);
  return rc;
}

