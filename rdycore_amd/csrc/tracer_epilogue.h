// The source epilogue and the stores of tracer_rhs_kernel and tracer_hr_kernel (tracer_kernels.h): both include this file behind
// their slot loop, with `constexpr bool HR` set.  Not a header of its own: no include guard, no namespace, and every name it
// uses -- NT, N, HR, a, t, dt, o, c, own, self, self_c, acc -- is the including kernel's.
// Included, not called: as a __device__ __forceinline__ function taking the bed slopes the same text contracts differently: the
// momentum components of F and u_out lose their bits in 33 of 56 test cases.  In place, the kernels' code is what it was.
    // ApplyTracerSourceSemiImplicit (tracer_petsc.c:617-737): bed slope, semi-implicit friction on the pre-source momentum sums,
    // erosion - deposition for wet cells.  ApplyTracerSourceHRSemiImplicit (1067-1154) is the same without the bed slope.
    const double h = own[0];
    const double n = a.mannings[o];
    double       bedx, bedy, tbx, tby;
    cell_source<RDYHIP_SOURCE_SEMI_IMPLICIT>(a, dt, h, own[1], own[2], acc[1], acc[2], HR ? 0.0 : a.dzdx[o], HR ? 0.0 : a.dzdy[o], n, bedx, bedy, tbx, tby);
    double F[N];
    F[0] = acc[0] + a.extsrc[3 * (int64_t)o + 0];
    F[1] = acc[1] + (-bedx - tbx + a.extsrc[3 * (int64_t)o + 1]);
    F[2] = acc[2] + (-bedy - tby + a.extsrc[3 * (int64_t)o + 2]);
    const bool   cell_wet = h >= a.tiny_h;
    const double Cd       = GRAVITY * (n * n) * rcbrt(h);
    const double tau_b    = 0.5 * TRACER_RHO_WATER * Cd * (self.u * self.u + self.v * self.v);  // h >= tiny_h: self.u = hu / h
    const double ei       = TRACER_KP * (tau_b - TRACER_TAU_EROSION) / TRACER_TAU_EROSION;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double di = TRACER_SETTLING * self_c[j] * (1.0 - tau_b / TRACER_TAU_DEPOSITION);
      F[3 + j]        = cell_wet ? acc[3 + j] + ((ei - di) + t.src[NT * (int64_t)o + j]) : acc[3 + j];
    }

    if (t.f) {
#pragma unroll
      for (int k = 0; k < N; ++k) RDY_ST(&t.f[N * (int64_t)o + k], F[k]);
    }
    // primitive variables (tracer_petsc.c:715-724): the regularised velocities, c_i = h c_i / h, all zero below tiny_h
    if (t.pv) {
      const RiemannSide p = riemann_side(h, own[1], own[2], a.tiny_h, a.h_anuga_sq);
      RDY_ST(&t.pv[N * (int64_t)o + 0], h);
      RDY_ST(&t.pv[N * (int64_t)o + 1], p.u);
      RDY_ST(&t.pv[N * (int64_t)o + 2], p.v);
#pragma unroll
      for (int j = 0; j < NT; ++j) RDY_ST(&t.pv[N * (int64_t)o + 3 + j], self_c[j]);
    }
    if (t.u_out) {
#pragma unroll
      for (int k = 0; k < N; ++k) RDY_ST(&t.u_out[N * c + k], fma(dt, F[k], own[k]));
    }
