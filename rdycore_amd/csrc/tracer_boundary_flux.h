// The boundary slot of tracer_rhs_kernel and tracer_hr_kernel (tracer_kernels.h) up to the edge's flux: both include this file
// in the `else` of `if (nid >= 0)`.  Not a header of its own: no include guard, no namespace, and every name it uses -- NT, N,
// UPWIND, a, t, btype, nid, self, self_c, sn, cn, fl, amax -- is the including kernel's.  It leaves k, R and cr to the kernel,
// which stores fl into bflux and tests the edge for wetness in its own order.
// Included, not called: as a __device__ __forceinline__ function (the ghost state alone, or with the flux) the same text
// contracts differently in tracer_hr_kernel -- tracer F differs in the last bit -- and with the flux inside, two
// instantiations take 8 VGPRs more and lose a wave per SIMD.
        // ApplyTracerBoundaryFlux (tracer_petsc.c:405-525): the cell is the left one.  Critical outflow is refused at
        // rdyhip_tracers_enable (472-474), so a type that is not Dirichlet is reflecting.  HR is a no-op here
        // (operator_fluxes_petsc.c:79-93): the own cell keeps the plain path's rule (h < tiny_h => 0, no regularisation).
        const int64_t k = -1 - nid;
        RiemannSide   R;
        double        cr[NT];
        if (btype[k] == RDYHIP_CONDITION_DIRICHLET) {
          double bv[N];
#pragma unroll
          for (int q = 0; q < N; ++q) bv[q] = t.bvalues[N * k + q];
          R = riemann_side(bv[0], bv[1], bv[2], a.tiny_h, 0.0);
          tracer_concentrations<NT>(bv[0], bv + 3, a.tiny_h, cr);
        } else {  // ApplyTracerReflectingBC (362-395): h and c_i copied, the velocity mirrored
          const double dum1 = sn * sn - cn * cn;
          const double dum2 = 2.0 * sn * cn;
          R.h               = self.h;
          R.u               = self.u * dum1 - self.v * dum2;
          R.v               = -self.u * dum2 - self.v * dum1;
          R.sqh             = self.sqh;
          R.c               = self.c;
#pragma unroll
          for (int j = 0; j < NT; ++j) cr[j] = self_c[j];
        }
        amax = tracer_roe_flux<NT, UPWIND>(self, R, self_c, cr, sn, cn, fl);
