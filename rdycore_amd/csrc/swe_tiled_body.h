// The body of the first-order / HR tiled kernels: the statements of swe_rhs_tiled_kernel and swe_rhs_ntab_kernel
// (swe_kernels.h), which include this file between their braces with `constexpr bool NTAB` set.  Not a header of its own: no
// include guard, no namespace, and every name it uses -- the template parameters S, SRC, OVW, HR, EULER, FNT, the kernel
// arguments a, dt, u, f -- is the including kernel's.
  // edge-record rounds held in registers: every tile has <= TILE_MAX_REC = 2 x 256 edge records (a 256-cell tile of a
  // well-numbered triangle mesh 1.6 per cell; a quad tile is cut at 240 cells, a 16 x 15 block = 511 records; round 4 ran
  // 256-cell quad tiles, 544 records, with a third round in which 32 of 256 lanes had work)
  constexpr bool HR_STAGED_VEL = HR;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int nside = S == 3 ? TILED_NS_TRI : TILED_NS_QUAD, nedge = TILED_NE;
  double   *sd_h = lds, *sd_u = lds + nside, *sd_v = lds + 2 * nside, *sd_sq = lds + 3 * nside, *sd_c = lds + 4 * nside;
  double   *sd_hu = lds + 5 * nside, *sd_hv = sd_hu + TILE;
  double   *ef0 = sd_hv + TILE, *ef1 = ef0 + nedge, *ef2 = ef1 + nedge, *eam = ef2 + nedge;
  // HR only: bed elevation per slot; per edge the momentum flux as the RIGHT cell sees it (ef1 / ef2 then hold the left
  // cell's: the Roe flux plus each side's own pressure correction)
  double   *sd_zc = eam + nedge, *efr1 = sd_zc + nside, *efr2 = efr1 + nedge;
  const int tid = threadIdx.x;
  // NTAB: the table's (cn, sn) pairs behind the last plane (tiled_ntab_lds_bytes), one lane per entry.  Phase 1 of the first
  // tile is the first reader, behind the loop's first barrier; nothing writes them again.
  //      Alignment: a pair is read with one 16-byte LDS instruction, so `lds` is declared aligned(16) -- the dynamic LDS then
  // starts on a multiple of 16 B whatever static __shared__ words the kernel has ahead of it (s_max / s_pos of
  // block_courant_reduce today) -- and tile_format.h asserts that the planes ahead of the table are a multiple of 16 B.  The
  // second-order kernels declare the same array (muscl_kernels.h) and carry the same attribute: one declaration per name.
  //      (The streamed instantiation computes `ntab` and never uses it; the table one carries cs0 / cs1 / ncs0 / ncs1 and
  // do_edge's `cs` as constants nobody reads.  Both fold away; declaring them per family would need a second copy of the
  // lines that rotate them.)
  typedef double NormalPair __attribute__((ext_vector_type(2)));
  NormalPair *const ntab = reinterpret_cast<NormalPair *>(lds + tiled_lds_bytes(S, HR) / sizeof(double));
  if constexpr (NTAB) {
    if (tid < RDY_COLD(a, nt_count)) {
      double cn, sn;
      edge_normal(a.cold->nt_flags[tid], a.cold->nt_cs[tid], cn, sn);
      NormalPair p;
      p.x       = cn;
      p.y       = sn;
      ntab[tid] = p;
    }
  }

  // ---- this workgroup's tile sequence.  Block ids are dealt round-robin to the
  // 8 XCDs: give each XCD a contiguous range of tiles and let its workgroups
  // interleave inside it, so concurrently running tiles are neighbours and
  // their halo cells hit that XCD's own L2.
  //      Dynamic walk (a.tile_walk, PHASE_ALL launches with xcd_chunks > 0): a workgroup's first three tiles are the static
  // walk's -- what the pipeline holds before a draw can have come back, so that no workgroup waits for a counter at the start
  // of the launch, when all of them would ask at once.  Every later index of the XCD's range comes from the XCD's counter
  // (ColdArgs::tile_draw), which hands out range start + 3 per_xcd + n in order to whichever workgroup asks next: tiles are
  // still taken in increasing order by workgroups that run side by side, and a workgroup that was held up takes fewer of
  // them instead of finishing last.  A draw is one returning atomic add by thread 0, issued with a tile's load batch for the
  // tile THREE ahead; it lands under the wait on the tile's streams behind the second barrier (a vmcnt(0)), where thread 0
  // leaves it in an LDS word (in the last, unused entry of eam[]: a tile has <= TILE_MAX_REC records); all waves read the
  // word after the next tile's first barrier, where the static walk computes idx2.  No barrier and no wait is added to the loop.
  int idx, step, hi;
  // The counter as a GLOBAL address: through a generic pointer the draw is a flat atomic, which every lgkmcnt wait of the
  // batch -- scalar loads, LDS -- waits for as well.
  typedef __attribute__((address_space(1))) int *DrawCtr;
  // (and as an address the compiler takes for divergent: for a uniform one it counts the active lanes, adds the count and
  // works each lane's value out of the result -- which it then waits for on the spot, in the middle of the load batch)
  // (the addend made where it is used: as a constant hipcc keeps it in a VGPR of its own for the whole launch)
  auto draw = [](int *ctr, int word) -> int {
    int one = 1;
    asm volatile("" : "+v"(word), "+v"(one));
    return __hip_atomic_fetch_add((DrawCtr)(uintptr_t)ctr + word, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  constexpr bool DYN   = tiled_has_dynamic_walk(S, SRC, HR, EULER);
  const bool     dyn   = DYN && a.tile_walk == TILE_WALK_DYNAMIC;  // uniform
  int *const draw_word = reinterpret_cast<int *>(eam + nedge - 1);
  if (a.xcd_chunks > 0) {
    const int x = blockIdx.x & 7;
    step        = gridDim.x >> 3;
    idx         = x * a.xcd_chunks + (blockIdx.x >> 3);
    hi          = min((x + 1) * a.xcd_chunks, a.n_work);
    // Draw n is tile n behind the XCD's first 3 per_xcd: the tile index of draw 0 sits beside the word (the loop has no SGPR
    // to keep it in), and the "draw" the first tile's batch finds is the workgroup's static third tile.
    if (dyn && tid == 0) {
      draw_word[0] = (int)(blockIdx.x >> 3) - step;
      draw_word[1] = x * a.xcd_chunks + 3 * step;
    }
  } else {
    idx  = blockIdx.x;
    step = gridDim.x;
    hi   = a.n_work;
  }
  auto tile_at = [&](int i) -> int { return __builtin_amdgcn_readfirstlane(a.list ? load_uniform(a.list, i) : i); };
  auto tile_desc = [&](int t) -> TileDesc {
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i v = load_uniform(reinterpret_cast<const v4i *>(a.tiles), t);
    TileDesc  d;
    d.e_off = v.x; d.h_off = v.y; d.c_off = v.z; d.cnt = (uint32_t)v.w;
    return d;
  };
  // INTERIOR phase (skip) skips tiles with ghost-adjacent cells (wave-uniform).  (skip: from the kernarg segment where it is
  // used, not a lane mask held for the launch)
  auto next_valid = [&](int i, bool skip) -> int {
    if (skip) {
      while (i < hi && tile_desc(tile_at(i)).halo()) i += step;
    }
    return i;
  };

  CourantTrack trk;

  // (kernels with the dynamic walk read the launch's walk from the kernarg segment where they need it; the others hold the phase)
  auto skips = [&]() -> bool {
    if constexpr (DYN) return hot_kernargs()->a.tile_walk == TILE_WALK_STATIC_SKIP;
    else return a.phase == RDYHIP_PHASE_INTERIOR;
  };
  idx = next_valid(idx, skips());
  if (idx < hi) {
    // ---- prologue: everything tile T0 needs, and the halo ids of T1
    int      tile = tile_at(idx);
    TileDesc td = tile_desc(tile);
    double   pu0 = 0.0, pu1 = 0.0, pu2 = 0.0;  // own cell state of the tile being started
    double   ph0 = 0.0, ph1 = 0.0, ph2 = 0.0;  // state of this thread's halo cell
    double   pz = 0.0, phz = 0.0;              // HR: bed elevation of the own / halo cell
    uint32_t lr0 = 0, lr1 = 0;                 // the two rounds of edge records
    double   cs0 = 0.0, cs1 = 0.0;
    CellStreams<S> cur{};  // set once: a lane without a cell keeps what it has, nobody reads it (load_streams)
    uint32_t nlr0 = 0, nlr1 = 0;  // the next tile's records, loaded under the counts phase 1 tests: no per-tile reset either
    double   ncs0 = 0.0, ncs1 = 0.0;
    {
      const int o = td.c_off + tid;
      if (tid < td.nc()) {
        const int c = a.o2l ? a.o2l[o] : o;
        pu0 = u[3 * (int64_t)c + 0]; pu1 = u[3 * (int64_t)c + 1]; pu2 = u[3 * (int64_t)c + 2];
        if (HR) pz = a.zc_local[c];
      }
      if (tid < td.nh()) {
        const int hc = *lane_ptr(a.hcells + (int64_t)td.h_off, lane_bytes(tid, 2));
        ph0 = u[3 * (int64_t)hc + 0]; ph1 = u[3 * (int64_t)hc + 1]; ph2 = u[3 * (int64_t)hc + 2];
        if (HR) phz = a.zc_local[hc];
      }
      const int ne = td.ne();
      if constexpr (NTAB) load_record_words(a, td.e_off, ne, tid, lr0, lr1);
      else load_records(a, td.e_off, ne, tid, lr0, cs0, lr1, cs1);
      load_streams<S, HR>(stream_args(hot_kernargs()), td.c_off, tid, tid < td.nc(), cur);
    }
    int      idx1 = next_valid(idx + step, skips());
    int      tile1 = 0, hid1 = 0, c1 = 0;  // next tile: this thread's halo cell and own cell (local ids)
    TileDesc td1 = td;
    if (idx1 < hi) {
      tile1 = tile_at(idx1);
      td1   = tile_desc(tile1);
      if (tid < td1.nh()) hid1 = *lane_ptr(a.hcells + (int64_t)td1.h_off, lane_bytes(tid, 2));
      const int o1 = td1.c_off + tid;
      c1           = (a.o2l && tid < td1.nc()) ? a.o2l[o1] : o1;
    }
    // The prologue's state, records and ids are waited for HERE, once per workgroup.  Left to the first use inside the loop
    // (phase 0), the wait would stand at the top of every tile -- hipcc orders the prologue's loads as it likes, so it is a
    // vmcnt(0) -- and drain the streams issued at the end of the previous tile before they had any time at all.
    if constexpr (NTAB)
      asm volatile("" ::"v"(pu0), "v"(pu1), "v"(pu2), "v"(ph0), "v"(ph1), "v"(ph2), "v"(pz), "v"(phz), "v"(lr0), "v"(lr1), "v"(hid1), "v"(c1));
    else
      asm volatile("" ::"v"(pu0), "v"(pu1), "v"(pu2), "v"(ph0), "v"(ph1), "v"(ph2), "v"(pz), "v"(phz), "v"(lr0), "v"(lr1), "v"(cs0), "v"(cs1), "v"(hid1),
                   "v"(c1));

    while (true) {
      // the walk and its counters: asked for here, used in the load batch behind the first barrier
      int  walk_t = TILE_WALK_STATIC;
      int *ctr_t  = nullptr;
      if constexpr (DYN) {
        const HotArgs hw = hot_kernargs();
        walk_t           = hw->a.tile_walk;
        ctr_t            = load_uniform(&hw->a.cold->tile_draw, 0);
      }
      // ... and the owned -> local map the batch looks the cells of the tile after the next up in: asked for with them, a
      // phase 0 ahead of its use.  (Held for the launch, the pointer and its null test are SGPRs that the tie path of phase 2
      // has to restore from VGPR lanes.)
      const int32_t *const o2l_hot = hot_kernargs()->a.o2l;
      const int  ne = td.ne(), nh = td.nh();
      const int  o      = td.c_off + tid;
      const bool active = tid < td.nc();

      // ---- phase 0: Riemann side data of the tile's own and halo cells -> LDS
      {
        RiemannSide self;
        self.h = self.u = self.v = self.sqh = self.c = 0.0;
        if (active) self = riemann_side(pu0, pu1, pu2, a.tiny_h, a.h_anuga_sq);
        if (HR_STAGED_VEL) hr_velocity_rule(self, a.tiny_h);
        sd_h[tid] = self.h; sd_u[tid] = self.u; sd_v[tid] = self.v; sd_sq[tid] = self.sqh; sd_c[tid] = self.c;
        sd_hu[tid] = pu1;
        sd_hv[tid] = pu2;
        if (HR) sd_zc[tid] = pz;
        if (tid < nh) {
          RiemannSide hs = riemann_side(ph0, ph1, ph2, a.tiny_h, a.h_anuga_sq);
          if (HR_STAGED_VEL) hr_velocity_rule(hs, a.tiny_h);
          sd_h[TILE + tid] = hs.h; sd_u[TILE + tid] = hs.u; sd_v[TILE + tid] = hs.v; sd_sq[TILE + tid] = hs.sqh; sd_c[TILE + tid] = hs.c;
          if (HR) sd_zc[TILE + tid] = phz;
        }
      }
      __syncthreads();

      // ---- software pipeline: the cell states and edge records of the next tile and the halo ids of the
      // one after are issued here in one batch (its per-cell streams follow at the end of this tile).
      // hipcc waits with s_waitcnt vmcnt(0) wherever a loaded register is first used, so nothing this
      // batch loads is used until the register rotation at the very end.  Two waits per tile on the hot
      // path: the one on this tile's streams after the second barrier -- a whole flux phase after this
      // batch was issued; it is a vmcnt(0) too, every load of the batch sits under a predicate and hipcc
      // can count none of them as issued (the branch-free form that lets it wait with vmcnt(8) was
      // timed: 1.3 % slower, profiles/RESULTS_LOG.md section 15) -- and the one at the end of the tile.
      // (a) which tile comes after the next, and the ids it needs (the only dependent loads: first)
      __builtin_amdgcn_s_setprio(3);  // waves that reach their load batch issue it ahead of waves that are computing (+0.7..1 %)
      int      idx2 = hi, tile2 = 0, hid2 = 0, c2 = 0;
      int      drawn = 0;  // thread 0, dynamic walk: the index of the tile after idx2
      TileDesc td2 = td1;
      if (idx1 < hi) {
        if (DYN && walk_t == TILE_WALK_DYNAMIC) {
          const int2 w = *reinterpret_cast<const int2 *>(draw_word);  // (draw, tile index of draw 0)
          idx2         = __builtin_amdgcn_readfirstlane(w.x) + __builtin_amdgcn_readfirstlane(w.y);
        } else {
          if constexpr (DYN) idx2 = next_valid(idx1 + step, walk_t == TILE_WALK_STATIC_SKIP);
          else idx2 = next_valid(idx1 + step, skips());
        }
        if (idx2 < hi) {
          // (not past a draw that came back beyond the range: every later one would too)
          if (DYN && walk_t == TILE_WALK_DYNAMIC && tid == 0) drawn = draw(ctr_t, (blockIdx.x & 7) * TILE_DRAW_STRIDE);
          tile2 = tile_at(idx2);
          td2   = tile_desc(tile2);
          if (tid < td2.nh()) hid2 = *lane_ptr(a.hcells + (int64_t)td2.h_off, lane_bytes(tid, 2));
          const int o2 = td2.c_off + tid;
          c2           = (o2l_hot && tid < td2.nc()) ? o2l_hot[o2] : o2;
        }
      }
      // (b) the next tile's cell states, edge records and per-cell streams
      if (idx1 < hi) {
        const double *const ub = hot_kernargs()->u;  // fetched beside the tile descriptor, not held across the loop
        if (tid < td1.nc()) {
          pu0 = ub[3 * (int64_t)c1 + 0]; pu1 = ub[3 * (int64_t)c1 + 1]; pu2 = ub[3 * (int64_t)c1 + 2];
          if (HR) pz = a.zc_local[c1];
        }
        if (tid < td1.nh()) {
          ph0 = ub[3 * (int64_t)hid1 + 0]; ph1 = ub[3 * (int64_t)hid1 + 1]; ph2 = ub[3 * (int64_t)hid1 + 2];
          if (HR) phz = a.zc_local[hid1];
        }
        const int ne1 = td1.ne();
        if constexpr (NTAB) load_record_words(a, td1.e_off, ne1, tid, nlr0, nlr1);
        else load_records(a, td1.e_off, ne1, tid, nlr0, ncs0, nlr1, ncs1);
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- phase 1: every edge of the tile once, operands from LDS only
      // (ApplyInteriorFlux / ApplyBoundaryFlux, swe_petsc.c:215-316, 506-630)
      auto do_edge = [&](int e, uint32_t lr, double cs) {
        double cn, sn;
        if constexpr (NTAB) {
          const NormalPair p = ntab[lr >> EDGE_NT_SHIFT];
          cn                 = p.x;
          sn                 = p.y;
        } else {
          edge_normal(lr, cs, cn, sn);
        }
        const int   jl = lr & EDGE_SLOT_MASK;
        RiemannSide L;
        L.h = sd_h[jl]; L.u = sd_u[jl]; L.v = sd_v[jl]; L.sqh = sd_sq[jl]; L.c = sd_c[jl];
        RoeFlux fl;
        bool    wet;
        if (!(lr & EDGE_BOUNDARY)) {
          const int   jr = (lr >> EDGE_R_SHIFT) & EDGE_SLOT_MASK;
          RiemannSide R;
          R.h = sd_h[jr]; R.u = sd_u[jr]; R.v = sd_v[jr]; R.sqh = sd_sq[jr]; R.c = sd_c[jr];
          if (!HR) {
            fl  = roe_flux(L, R, sn, cn);
            wet = !(R.h < a.tiny_h && L.h < a.tiny_h);
          } else {
            // hydrostatic reconstruction (swe_petsc.c:1046-1071); velocities are kept, with the strict
            // "h > tiny_h" wet test of the HR operator (1061-1064)
            const double zl = sd_zc[jl], zr = sd_zc[jr];
            RiemannSide  Lr, Rr;
            hr_reconstruct(L, R, zl, zr, Lr, Rr);
            fl     = roe_flux(Lr, Rr, sn, cn);
            const bool outer = !(R.h < a.tiny_h && L.h < a.tiny_h);       // 1094
            wet              = outer && (Lr.h > a.tiny_h || Rr.h > a.tiny_h);  // inner guard, 1112
            // pressure correction g (h^2 - h*^2) / 2 n of each side, applied whenever the outer guard holds (1136-1152), the
            // Roe flux only under the inner one: both folded into one momentum flux per side here, so that phase 2 reads
            // four values per slot instead of seven
            const double pl = outer ? 0.5 * GRAVITY * (L.h * L.h - Lr.h * Lr.h) : 0.0;
            const double pr = outer ? 0.5 * GRAVITY * (R.h * R.h - Rr.h * Rr.h) : 0.0;
            if (!wet) fl.f0 = fl.f1 = fl.f2 = 0.0;
            efr1[e] = fma(pr, cn, fl.f1);
            efr2[e] = fma(pr, sn, fl.f2);
            fl.f1   = fma(pl, cn, fl.f1);
            fl.f2   = fma(pl, sn, fl.f2);
          }
        } else {
          // boundary edges: HR is a no-op (operator_fluxes_petsc.c:57-58); their cell is the left one
          const int    k  = RDY_COLD(a, tile_bk)[load_uniform(RDY_COLD(a, tile_boff), tile) + ((lr >> EDGE_R_SHIFT) & EDGE_SLOT_MASK)];
          if (HR_STAGED_VEL && L.h == a.tiny_h) {
            // the staged velocities carry the HR operator's "h > tiny_h" rule, ApplyBoundaryFlux wants ComputeRiemannVelocities'
            // "h < tiny_h => 0" (swe_petsc.c:62): they differ at equality only (the left cell of a boundary edge is a tile cell)
            const RiemannSide s = riemann_side(L.h, sd_hu[jl], sd_hv[jl], a.tiny_h, a.h_anuga_sq);
            L.u = s.u;
            L.v = s.v;
          }
          BoundaryFlux bf = boundary_flux(RDY_COLD(a, btype)[k], true, L, RDY_COLD(a, bvalues) + 3 * (int64_t)k, sn, cn, a.tiny_h, a.h_anuga_sq);
          fl              = bf.flux;
          wet             = bf.wet;
          store_boundary_flux(a, k, fl, dt);
          if (HR) {
            if (!wet) fl.f0 = fl.f1 = fl.f2 = 0.0;  // phase 2 of the HR variant adds every edge's flux
            // a boundary edge has no right cell, but phase 2 picks the side by the sign of the slot's coefficient: keep the
            // right-hand copy defined too (never stale LDS of the previous tile, whatever the coefficient's sign bit says)
            efr1[e] = fl.f1;
            efr2[e] = fl.f2;
          }
        }
        ef0[e] = fl.f0;
        ef1[e] = fl.f1;
        ef2[e] = fl.f2;
        eam[e] = wet ? fl.amax : -1.0;  // -1 marks a dry-dry edge (skipped, swe_petsc.c:285)
      };
      // Both rounds take their records from registers.  This loop must contain no global load on any
      // path: hipcc would put an s_waitcnt vmcnt(0) at the merge, and every round would then wait for
      // the whole prefetch batch issued above.
#pragma unroll 1
      for (int r = 0; r < 2; ++r) {
        const int e = tid + r * TILE;
        if (e < ne) do_edge(e, r == 0 ? lr0 : lr1, r == 0 ? cs0 : cs1);
      }
      __syncthreads();
      // The tile's wait on its per-cell streams, once, ahead of every use: they were issued at the end of the previous tile
      // (the first tile's in the prologue), before that tile's stores and this tile's batch.
      if constexpr (DYN)
        asm volatile("" ::"v"(cur.r0), "v"(cur.r1), "v"(cur.coef[0]), "v"(cur.coef[1]), "v"(cur.coef[2]), "v"(cur.coef[S - 1]), "v"(cur.dzdx),
                     "v"(cur.dzdy), "v"(cur.nman), "v"(cur.s0), "v"(cur.s1), "v"(cur.s2), "v"(drawn));
      else
        asm volatile("" ::"v"(cur.r0), "v"(cur.r1), "v"(cur.coef[0]), "v"(cur.coef[1]), "v"(cur.coef[2]), "v"(cur.coef[S - 1]), "v"(cur.dzdx),
                     "v"(cur.dzdy), "v"(cur.nman), "v"(cur.s0), "v"(cur.s1), "v"(cur.s2));
      // That wait is a vmcnt(0): the draw issued with the batch has landed too.  Thread 0 leaves it for the next tile's batch
      // here, behind the second barrier (under the static walk it is a zero nobody reads), and the register is free for phase 2.
      if (DYN && tid == 0) draw_word[0] = drawn;
      // what the end of the tile reads once -- the stream arrays of the next tile's loads, the output arrays -- comes from the
      // kernarg segment here, a whole phase 2 ahead of its use
      const HotArgs    hk = hot_kernargs();
      const StreamArgs sa = stream_args(hk);
      double *const    f_hot = hk->f, *const pv_hot = hk->a.pv, *const fdiv_hot = hk->a.fdiv, *const uout_hot = hk->a.u_out;

      // ---- phase 2: per-cell sum in the reference's edge order, source terms; the stores come last
      double out[6];       // F[3], then the primitive variables (h, u, v)
      double acc_fdiv[3];
      double own_hu, own_hv;  // EULER only
      rows_unset(out, acc_fdiv, own_hu, own_hv);
      if (active) {
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
        if (!OVW) {  // ApplyOperator semantics: add into f (and let the friction term see it)
          acc0 = f[3 * (int64_t)o + 0];
          acc1 = f[3 * (int64_t)o + 1];
          acc2 = f[3 * (int64_t)o + 2];
        }
        bool      tie      = false;  // a slot of this cell met the thread's running Courant maximum to the last bit
        const int rec_in   = trk.rec;
        // The LDS reads of phase 2 in ONE batch with one wait: the S wave speeds, the 3 S fluxes and the lane's own depth and
        // velocities.  All addresses are known once the slot words are in registers; read where they are used, each value cost
        // a round trip of its own (the guards below sit between them), ten in series for a triangle's twelve values.  An
        // empty slot reads the last record's entry of each plane (in bounds: a tile has <= TILE_MAX_REC records); nobody looks
        // at what it gets.  The guards and the sums stay what they were.
        //      The lane's own momenta are NOT in the batch: cell_results reads them where it did.  As values of another block,
        // hipcc contracts the friction term's u u + v v the other way round -- fma(u, u, v v) for fma(v, v, u u) -- and a
        // cell in ten thousand gets another last bit.
        uint32_t refs[S];
        double   ams[S], e0[S], e1[S], e2[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if (S == 3) {
            refs[s] = (cur.r0 >> (10 * s)) & 0x3FF;
          } else {
            const uint32_t w = (s < 2) ? cur.r0 : cur.r1;
            refs[s]          = (s & 1) ? (w >> 16) : (w & 0xFFFFu);
          }
          const uint32_t j = refs[s] & (uint32_t)(TILE_MAX_REC - 1);
          ams[s]           = eam[j];
          e0[s]            = ef0[j];
          if (HR) {
            const bool left = __builtin_signbit(cur.coef[s]);  // this cell is the edge's left (k = -len/area, -0.0 for a degenerate edge) or right cell
            e1[s]           = (left ? ef1 : efr1)[j];
            e2[s]           = (left ? ef2 : efr2)[j];
          } else {
            e1[s] = ef1[j];
            e2[s] = ef2[j];
          }
        }
        const double self_h = sd_h[tid], self_u = sd_u[tid], self_v = sd_v[tid];
        asm volatile("" ::"v"(ams[0]), "v"(ams[1]), "v"(ams[2]), "v"(ams[S - 1]), "v"(e0[0]), "v"(e0[1]), "v"(e0[2]), "v"(e0[S - 1]), "v"(e1[0]),
                     "v"(e1[1]), "v"(e1[2]), "v"(e1[S - 1]), "v"(e2[0]), "v"(e2[1]), "v"(e2[2]), "v"(e2[S - 1]), "v"(self_h), "v"(self_u),
                     "v"(self_v));
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const uint32_t ref = refs[s];
          if (ref == (S == 3 ? REF3_EMPTY : (uint32_t)SLOT_EMPTY)) continue;
          const double am = ams[s];
          const double k  = cur.coef[s];
          if (HR) {
            // a dry-dry edge (am == -1) carries zero Roe flux here but still its pressure correction
            acc0 += e0[s] * k;
            acc1 += e1[s] * k;
            acc2 += e2[s] * k;
          }
          if (am != -1.0) {
            // (in the arm of the Courant compares: in an arm of their own, now that they load nothing, hipcc runs the three
            // fma for every slot and picks with six v_cndmask)
            if (!HR) {
              acc0 += e0[s] * k;
              acc1 += e1[s] * k;
              acc2 += e2[s] * k;
            }
            // len/area_self: the max over an edge's two cells is len / min(area_l, area_r) (swe_petsc.c:289)
            const double cnum = am * fabs(k) * dt;
            tie |= cnum == trk.best;
            if (cnum > trk.best) {
              trk.best = cnum;
              trk.rec  = td.e_off + (int)ref;
            }
          }
        }
        if (trk.rec != rec_in) trk.pos = -1;
        // cold: which of the equal edges comes first in the reference's loop (CourantTrack).  Dismissed at once where the
        // incumbent's position is known and smaller than every position of this tile.  The tile's two bounds -- the loop
        // positions of its records 0 and COURANT_Q (sorted by position) -- are read HERE, with scalar loads, by the waves
        // that have a tie: fetched a tile ahead and rotated with the pipeline they were two scalars live across the whole
        // loop, which cost every tile more than this path costs the few that take it.
        int pos_lo = 0, pos_q = 0;
        if (tie) {
          const int32_t *e_pos = RDY_COLD(a, e_pos);
          pos_lo               = load_uniform(e_pos, td.e_off);
          pos_q                = load_uniform(e_pos, td.e_off + min(COURANT_Q, ne - 1));
        }
        if (tie && !(trk.pos >= 0 && trk.pos < pos_lo)) {
          int first = -1;  // the first slot of this cell at the running maximum: the only one that can come before the incumbent
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const uint32_t ref = refs[s];
            if (ref == (S == 3 ? REF3_EMPTY : (uint32_t)SLOT_EMPTY)) continue;
            // the batch's value, nothing has written the plane since: no round trip here either.  (Taken as a value of its own:
            // left to merge this path's products with the slot loop's, hipcc keeps those alive across the branch for a path
            // almost no tile takes.)
            double am = ams[s];
            asm volatile("" : "+v"(am));
            if (first < 0 && am != -1.0 && am * fabs(cur.coef[s]) * dt == trk.best) first = (int)ref;
          }
          if (first >= 0) courant_resolve_tie(a, trk, td.e_off + first, first >= COURANT_Q ? pos_q : pos_lo);
        }
        acc_fdiv[0] = acc0;
        acc_fdiv[1] = acc1;
        acc_fdiv[2] = acc2;
        cell_results<SRC>(a, dt, self_h, sd_hu[tid], sd_hv[tid], acc0, acc1, acc2, cur.dzdx, cur.dzdy, cur.nman, cur.s0, cur.s1, cur.s2, out);
        out[3] = self_h;
        out[4] = self_u;
        out[5] = self_v;
        if (HR_STAGED_VEL && out[3] == a.tiny_h) {  // primitive variables: zero BELOW tiny_h (swe_petsc.c:788-791), see hr_velocity_rule
          const RiemannSide s = riemann_side(out[3], sd_hu[tid], sd_hv[tid], a.tiny_h, a.h_anuga_sq);
          out[4] = s.u;
          out[5] = s.v;
        }
        if (EULER) {
          own_hu = sd_hu[tid];
          own_hv = sd_hv[tid];
        }
      }
      const bool last = idx1 >= hi;
      // The tile's wait on the prefetch batch: its youngest load is "used" here, before this tile's stores are
      // issued (vmcnt counts stores too, and the register rotation below is materialised at the very end of the
      // loop body).
      if constexpr (NTAB)
        asm volatile("" ::"v"(pu0), "v"(pu1), "v"(pu2), "v"(ph0), "v"(ph1), "v"(ph2), "v"(pz), "v"(phz), "v"(nlr0), "v"(nlr1), "v"(hid2), "v"(c2));
      else
        asm volatile("" ::"v"(pu0), "v"(pu1), "v"(pu2), "v"(ph0), "v"(ph1), "v"(ph2), "v"(pz), "v"(phz), "v"(nlr0), "v"(nlr1), "v"(ncs0), "v"(ncs1),
                     "v"(hid2), "v"(c2));
      // rotate the pipeline registers, store
      const bool send_tile = EULER && td.send();  // wave-uniform
      const int  tile_cur  = tile, nc_cur = td.nc(), c_off_cur = td.c_off;
      idx = idx1; tile = tile1; td = td1;
      idx1 = idx2; tile1 = tile2; td1 = td2; hid1 = hid2; c1 = c2;
      lr0 = nlr0; lr1 = nlr1; cs0 = ncs0; cs1 = ncs1;
      // the next tile's per-cell streams, into the registers phase 2 (its cold Courant tie path included) has just read
      // for the last time; not on the workgroup's last tile
      load_streams<S, HR>(sa, td.c_off, tid, !last && tid < td.nc(), cur);
      __builtin_amdgcn_sched_barrier(0);
      // F, pv (and fdiv, u_out) are [cell][3]: a wave's 64 cells own 192 consecutive doubles of each.  The rows are
      // transposed through wave shuffles so that every store instruction writes 512 contiguous bytes (whole lines)
      // instead of 64 x 8 bytes at a 24-byte stride -- with the non-temporal hint the strided partial lines reach HBM
      // unmerged (0.58 GB written for 0.48 GB of output).  All 64 lanes take part, cells past the end are masked.
      {
        const int      lane  = tid & 63;
        const int64_t  row0  = 3 * (int64_t)c_off_cur;  // the tile's first row: array + row0 is a scalar base
        const uint32_t rowb  = lane_bytes(3 * tid - 2 * lane, 3);
        const int      ncell = nc_cur - (tid - lane);  // the wave's cells of this tile
        // the transpose goes through the wave's own 64 entries of sd_v, sd_sq and sd_c (wave_store_rows3_lds): phase 1 read
        // them for the last time before the second barrier, out[5] has this lane's sd_v, phase 0 of the next tile rewrites them
        const RowTranspose rt = row_transpose_slots<nside>(sd_v + (tid - lane), lane);
        if (!EULER || f_hot) wave_store_rows3_lds<nside, FNT>(f_hot + row0, rowb, lane, ncell, rt, out[0], out[1], out[2]);
        // the primitive variables only once somebody has asked for them (KernelArgs::pv); a branch with ONE arm, like fdiv's
        if (pv_hot) wave_store_rows3_lds<nside>(pv_hot + row0, rowb, lane, ncell, rt, out[3], out[4], out[5]);
        if (fdiv_hot) wave_store_rows3_lds<nside>(fdiv_hot + row0, rowb, lane, ncell, rt, acc_fdiv[0], acc_fdiv[1], acc_fdiv[2]);
        if (EULER) {
          const double n0 = out[3] + dt * out[0], n1 = own_hu + dt * out[1], n2 = own_hv + dt * out[2];
          if (!a.o2l) {
            // u_out is what the NEXT step reads.  With the hint it is not in the Infinity Cache then; without it, it is -- if it
            // fits: a 2.8 M-cell part (67 MB of state) steps 8 % faster with plain stores, a 10 M-cell one (240 MB of a 256 MB
            // cache) 3.5 % slower (profiles/r04_uout_store_policy.txt).  FNT = false is the instantiation for states that fit.
            wave_store_rows3_lds<nside, FNT>(uout_hot + row0, rowb, lane, ncell, rt, n0, n1, n2);
          } else if (active) {  // owned cells are not a prefix of the local numbering: scattered rows
            const int64_t c = a.o2l[o];
            if constexpr (FNT) {
              RDY_ST(&uout_hot[3 * c + 0], n0);
              RDY_ST(&uout_hot[3 * c + 1], n1);
              RDY_ST(&uout_hot[3 * c + 2], n2);
            } else {
              uout_hot[3 * c + 0] = n0;
              uout_hot[3 * c + 1] = n1;
              uout_hot[3 * c + 2] = n2;
            }
          }
          if (send_tile) wave_store_send_rows(a, tile_cur, tid, n0, n1, n2);
        }
      }
      if (last) break;
    }
  }
  if (DYN && tid == 0 && hot_kernargs()->a.tile_walk == TILE_WALK_DYNAMIC) {
    // Every draw of this workgroup has returned.  The workgroup that leaves last puts the nine words back to zero for the
    // next launch (stores at the scope of the atomics): no reset launch, no host call.
    int *const ctr = load_uniform(&hot_kernargs()->a.cold->tile_draw, 0);
    if (atomicAdd(ctr + 8 * TILE_DRAW_STRIDE, 1) == (int)gridDim.x - 1) {
#pragma unroll
      for (int i = 0; i < 9; ++i) __hip_atomic_store(ctr + i * TILE_DRAW_STRIDE, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  courant_extra_edges<HR>(a, dt, u, trk);
  block_courant_reduce<TILE>(a, trk.best, RDY_COLD(a, e_pos), trk.rec);
