// The host-side layout pass of rdyhip_create / rdyhip_probe_layout: validation of the caller's mesh arrays and every table
// the kernels read.  No device call anywhere in this file, and no HIP header: it includes only rdyhip.h, tile_format.h,
// error.h and the standard library, so it also builds with a plain host compiler into a stand-alone program
// (tests/host/layout_dump.cpp, run under the address and undefined-behaviour sanitizers by tests/test_layout_tables_cpu.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

#include "rdyhip.h"
#include "error.h"
#include "tile_format.h"

namespace rdyhip {

// Everything rdyhip_create derives from the mesh on the host, before any device call: validation, the slot tables in the
// reference's loop order, the tiles with their edge records / halo lists / boundary lists, the second-order stencils.
// The numbers of a layout: what the operator keeps of it (RDyHipOperator_s derives from this) and what
// rdyhip_layout_info / rdyhip_probe_layout report
struct LayoutCounts {
  int32_t n_cells = 0, n_owned = 0, S = 3, K = 0, n_halo = 0, ntiles = 0, n_halo_tiles = 0, emax = 0, hmax = 0, hmax2 = 0;
  int64_t nrec = 0, nhalo_entries = 0, n_hcells2 = 0;
  bool    prefix = true, muscl = false;
  size_t  lds_bytes = 0, lds_muscl = 0;
};

struct HostLayout {
  int32_t nc = 0, no = 0, ne = 0, ni = 0, K = 0, S = 3, ntiles = 0, emax = 0, hmax = 0, hmax2 = 0;
  int64_t stride = 0;
  bool    prefix = true, hr_on = false, muscl_on = false;
  size_t  lds_bytes = 0, lds_muscl = 0;
  std::vector<int32_t>  o2l, boff, nbr, pos, btype, bleft, bedge, bghost, halo, hcells, tile_bk, tile_boff, tile_c0, halo_tiles, hcells2, c_off, e_pos;
  std::vector<double>   cn, sn, coef, bcn, bsn, e_cs, e_mid, dzdx, dzdy;
  std::vector<TileDesc> tiles;
  std::vector<uint32_t> e_lr;
  // the extra Courant edges (ColdArgs::x_*): internal edges the owned cells' slots do not cover as the reference's loop does
  std::vector<int32_t>  x_lr, x_pos;
  std::vector<uint32_t> x_flags;
  std::vector<double>   x_cs, x_cfac, x_mid;
  std::vector<uint16_t> slot_ref, bn_idx;
  std::vector<uint32_t> ref3;     // S == 3: the slot references as the kernels read them, 3 x 10 bits per owned cell
  std::vector<double>   cxy, zc;  // second order: cell centroids [nc][2]; HR: bed elevation per local cell
  LayoutCounts          counts;
};

// argument checks of rdyhip_create (the reference's PetscCheck messages where it has them)
static int layout_check_arguments(const RDyHipConfig *config, const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries) {
  if (!config || !mesh) return fail(RDYHIP_ERR_USER, "null argument to rdyhip_create");
  if (num_boundaries < 0 || (num_boundaries > 0 && !boundaries)) return fail(RDYHIP_ERR_USER, "bad boundary list");
  if (config->riemann != RDYHIP_RIEMANN_ROE) return fail(RDYHIP_ERR_USER, "Unsupported Riemann solver");  // swe_petsc.c:269
  if (config->source_method != RDYHIP_SOURCE_SEMI_IMPLICIT && config->source_method != RDYHIP_SOURCE_IMPLICIT_XQ2018)
    return fail(RDYHIP_ERR_USER, "Only semi_implicit and implicit_xq2018 are supported");  // swe_petsc.c:973
  if (config->well_balancing != RDYHIP_WELL_BALANCING_NONE && config->well_balancing != RDYHIP_WELL_BALANCING_HR)
    return fail(RDYHIP_ERR_USER, "Only well_balancing = none or hydrostatic_reconstruction is supported in the PETSc version");  // operator.c:388
  if (config->well_balancing == RDYHIP_WELL_BALANCING_HR && !mesh->cell_zc)
    return fail(RDYHIP_ERR_USER, "hydrostatic reconstruction needs the per-cell bed elevation (RDyHipMesh.cell_zc)");
  const bool muscl_on = config->second_order != 0;
  if (muscl_on && config->well_balancing == RDYHIP_WELL_BALANCING_HR)
    return fail(RDYHIP_ERR_USER, "-second_order cannot be used with well_balancing = HR simultaneously (not yet implemented)");  // operator.c:388-389
  if (muscl_on && config->limiter != RDYHIP_LIMITER_MINMOD && config->limiter != RDYHIP_LIMITER_NONE && config->limiter != RDYHIP_LIMITER_VANLEER)
    return fail(RDYHIP_ERR_USER, "unknown slope limiter %d", config->limiter);
  if (muscl_on && mesh->num_edges > 0 && (!mesh->cell_centroids || !mesh->edge_vertex_ids || !mesh->vertex_points))
    return fail(RDYHIP_ERR_USER, "second_order needs RDyHipMesh.cell_centroids, edge_vertex_ids and vertex_points");
  const int32_t nc = mesh->num_cells, no = mesh->num_owned_cells, ne = mesh->num_edges, ni = mesh->num_internal_edges;
  if (nc < 0 || no < 0 || no > nc || ne < 0 || ni < 0 || ni > ne) return fail(RDYHIP_ERR_ARG_SIZ, "inconsistent mesh sizes");
  if (nc >= NBR_GHOST) return fail(RDYHIP_ERR_ARG_SIZ, "too many local cells (%d) for the 30-bit neighbour encoding", nc);
  if (nc > 0 && (!mesh->cell_is_owned || !mesh->cell_local_to_owned || !mesh->cell_areas || !mesh->cell_dz_dx || !mesh->cell_dz_dy))
    return fail(RDYHIP_ERR_USER, "null cell array");
  if (ne > 0 && (!mesh->edge_cell_ids || !mesh->edge_lengths || !mesh->edge_cn || !mesh->edge_sn)) return fail(RDYHIP_ERR_USER, "null edge array");
  if (ni > 0 && !mesh->edge_internal_ids) return fail(RDYHIP_ERR_USER, "null internal edge list");

  return 0;
}

// owned <-> local maps, the boundary-edge table and the per-cell slot tables in the reference's loop order
// (with the least-squares gradient coefficients of the second-order path)
static int layout_build_slots(const RDyHipConfig *config, const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries,
                              HostLayout &L) {
  const bool    muscl_on = config->second_order != 0;
  const int32_t nc = mesh->num_cells, no = mesh->num_owned_cells, ne = mesh->num_edges, ni = mesh->num_internal_edges;
  // ---- owned <-> local maps ---------------------------------------------
  std::vector<int32_t> o2l((size_t)no, -1);
  int32_t              owned_seen = 0;
  for (int32_t c = 0; c < nc; ++c) {
    if (mesh->cell_is_owned[c]) {
      const int32_t o = mesh->cell_local_to_owned[c];
      if (o < 0 || o >= no || o2l[o] != -1) return fail(RDYHIP_ERR_USER, "cells.local_to_owned is not a bijection onto the owned cells");
      o2l[o] = c;
      ++owned_seen;
    }
  }
  if (owned_seen != no) return fail(RDYHIP_ERR_ARG_SIZ, "num_owned_cells (%d) does not match cells.is_owned (%d)", no, owned_seen);
  bool prefix = true;
  for (int32_t o = 0; o < no; ++o) prefix = prefix && (o2l[o] == o);

  // ---- boundary-edge table ------------------------------------------------
  std::vector<int32_t> boff((size_t)num_boundaries + 1, 0);
  for (int32_t b = 0; b < num_boundaries; ++b) {
    if (boundaries[b].num_edges < 0 || (boundaries[b].num_edges > 0 && !boundaries[b].edge_ids)) return fail(RDYHIP_ERR_USER, "bad boundary %d", b);
    const int32_t t = boundaries[b].condition_type;
    if (t != RDYHIP_CONDITION_DIRICHLET && t != RDYHIP_CONDITION_REFLECTING && t != RDYHIP_CONDITION_CRITICAL_OUTFLOW)
      return fail(RDYHIP_ERR_USER, "Invalid boundary condition encountered for boundary %d", b);  // swe_petsc.c:568
    boff[b + 1] = boff[b] + boundaries[b].num_edges;
  }
  const int32_t K = boff[num_boundaries];

  // ---- count slots per owned cell -----------------------------------------
  std::vector<int32_t> cnt((size_t)no, 0);
  for (int32_t p = 0; p < ni; ++p) {
    const int32_t e = mesh->edge_internal_ids[p];
    if (e < 0 || e >= ne) return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "internal edge id %d out of range", e);
    const int32_t l = mesh->edge_cell_ids[2 * e], r = mesh->edge_cell_ids[2 * e + 1];
    if (r == -1) continue;  // swe_petsc.c:249
    if (l < 0 || l >= nc || r < 0 || r >= nc) return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "edge %d has cell ids (%d,%d) out of range", e, l, r);
    if (mesh->cell_is_owned[l]) cnt[mesh->cell_local_to_owned[l]]++;
    if (mesh->cell_is_owned[r]) cnt[mesh->cell_local_to_owned[r]]++;
  }
  for (int32_t b = 0; b < num_boundaries; ++b) {
    for (int32_t i = 0; i < boundaries[b].num_edges; ++i) {
      const int32_t e = boundaries[b].edge_ids[i];
      if (e < 0 || e >= ne) return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "boundary %d edge id %d out of range", b, e);
      const int32_t l = mesh->edge_cell_ids[2 * e];
      if (l < 0 || l >= nc) return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "boundary edge %d has no left cell", e);
      if (mesh->cell_is_owned[l]) cnt[mesh->cell_local_to_owned[l]]++;
    }
  }
  int32_t maxcnt = 0;
  for (int32_t o = 0; o < no; ++o) maxcnt = std::max(maxcnt, cnt[o]);
  if (maxcnt > 4) return fail(RDYHIP_ERR_USER, "a cell has %d edges (must be 3 or 4)", maxcnt);  // rdymesh.c:809
  const int32_t S      = maxcnt <= 3 ? 3 : 4;
  const int64_t stride = ((int64_t)no + 63) / 64 * 64;

  // ---- fill slots in the reference's loop order ---------------------------
  std::vector<int32_t> nbr((size_t)(S * stride), NBR_EMPTY), pos((size_t)(S * stride), -1);
  std::vector<double>  cn((size_t)(S * stride), 0.0), sn((size_t)(S * stride), 0.0), coef((size_t)(S * stride), 0.0);
  std::fill(cnt.begin(), cnt.end(), 0);
  if (muscl_on) {
    // every internal edge needs both cells for the second-order stencils (src/operator_fluxes_ceed.c:897-901)
    for (int32_t p = 0; p < ni; ++p) {
      const int32_t e = mesh->edge_internal_ids[p];
      if (mesh->edge_cell_ids[2 * e + 1] == -1) return fail(RDYHIP_ERR_USER, "second_order: internal edge %d has no right cell", e);
    }
  }
  auto put = [&](int32_t o, int32_t id, double c, double s, double k, int32_t p) {
    const int64_t idx = (int64_t)cnt[o]++ * stride + o;
    nbr[idx]          = id;
    cn[idx]           = c;
    sn[idx]           = s;
    coef[idx]         = k;
    pos[idx]          = p;
  };
  for (int32_t p = 0; p < ni; ++p) {
    const int32_t e = mesh->edge_internal_ids[p];
    const int32_t l = mesh->edge_cell_ids[2 * e], r = mesh->edge_cell_ids[2 * e + 1];
    if (r == -1) continue;
    const double len = mesh->edge_lengths[e];
    if (mesh->cell_is_owned[l]) put(mesh->cell_local_to_owned[l], r | (mesh->cell_is_owned[r] ? 0 : NBR_GHOST), mesh->edge_cn[e], mesh->edge_sn[e], -len / mesh->cell_areas[l], p);
    if (mesh->cell_is_owned[r]) put(mesh->cell_local_to_owned[r], l | (mesh->cell_is_owned[l] ? 0 : NBR_GHOST), mesh->edge_cn[e], mesh->edge_sn[e], len / mesh->cell_areas[r], p);
  }
  std::vector<int32_t> btype((size_t)K), bleft((size_t)K), bedge((size_t)K), bghost;
  std::vector<double>  bcn((size_t)K), bsn((size_t)K);
  for (int32_t b = 0; b < num_boundaries; ++b) {
    for (int32_t i = 0; i < boundaries[b].num_edges; ++i) {
      const int32_t k = boff[b] + i;
      const int32_t e = boundaries[b].edge_ids[i];
      const int32_t l = mesh->edge_cell_ids[2 * e];
      btype[k]        = boundaries[b].condition_type;
      bleft[k]        = l;
      bedge[k]        = e;
      bcn[k]          = mesh->edge_cn[e];
      bsn[k]          = mesh->edge_sn[e];
      if (mesh->cell_is_owned[l]) put(mesh->cell_local_to_owned[l], -1 - k, mesh->edge_cn[e], mesh->edge_sn[e], -mesh->edge_lengths[e] / mesh->cell_areas[l], ni + k);
      else bghost.push_back(k);
    }
  }
  // owned cells with a ghost neighbour
  std::vector<int32_t> halo;
  for (int32_t o = 0; o < no; ++o) {
    bool g = false;
    for (int32_t s = 0; s < S; ++s) {
      const int32_t id = nbr[(int64_t)s * stride + o];
      g                = g || (id >= 0 && (id & NBR_GHOST));
    }
    if (g) halo.push_back(o);
  }

  L.nc = nc; L.no = no; L.ne = ne; L.ni = ni; L.K = K; L.S = S; L.stride = stride; L.prefix = prefix; L.muscl_on = muscl_on;
  L.o2l = std::move(o2l); L.boff = std::move(boff); L.nbr = std::move(nbr); L.pos = std::move(pos); L.btype = std::move(btype);
  L.bleft = std::move(bleft); L.bedge = std::move(bedge); L.bghost = std::move(bghost); L.halo = std::move(halo);
  L.cn = std::move(cn); L.sn = std::move(sn); L.coef = std::move(coef);
  L.bcn = std::move(bcn); L.bsn = std::move(bsn);
  return 0;
}

// Where the tiles end.  A tile is a run of consecutive owned cells, at most `max_cells` (<= TILE) of them, grown 16 cells
// at a time (whole 128-byte lines of the [cell][3] outputs) while it fits the kernels' fixed capacities: TILE_MAX_REC edge
// records (two register rounds of the edge phase), the halo-cell planes in LDS and, for second order, the two rings.  Nothing
// else ends a tile (round 5 first also ended one where 16 cells shared no edge with it -- "the numbering jumps" -- which cut
// the nested numbering of a refined mesh into 64-cell tiles: 2.3 x slower, profiles/RESULTS_LOG.md section 12).  Any numbering
// is accepted; one without locality gets small tiles (a random one: ~30 cells) and runs slowly, correctly.
// Returns the first owned cell of every tile, [ntiles + 1].
static std::vector<int32_t> layout_cut_tiles(const RDyHipMesh *mesh, const HostLayout &L, int32_t max_cells) {
  const int32_t nc = L.nc, no = L.no, S = L.S, npos = L.ni + L.K;
  const int64_t stride = L.stride;
  const auto   &nbr = L.nbr;
  const auto   &pos = L.pos;
  const int32_t max_rec = TILE_MAX_REC, max_h1 = S == 3 ? TILE_MAX_HALO_TRI : TILE_MAX_HALO_QUAD;
  const int32_t max_ring = S == 3 ? MUSCL_MAX_RING_TRI : MUSCL_MAX_RING_QUAD;
  std::vector<int32_t> c0;
  c0.reserve((size_t)no / 200 + 2);
  // stamps: edge positions in the tile / in the candidate granule; cells in the first ring / candidates / second ring
  std::vector<int32_t> emark((size_t)npos, -1), etry((size_t)npos, -1), r1mark((size_t)nc, -1), r1try((size_t)nc, -1), r2try((size_t)nc, -1);
  std::vector<int32_t> r1, r1new;
  int32_t stamp = 0, attempt = 0;
  int32_t base = 0;
  while (base < no) {
    c0.push_back(base);
    ++stamp;
    r1.clear();
    int32_t cells = 0, rec = 0;
    int32_t gran = 16;
    while (cells < max_cells && base + cells < no) {
      const int32_t g = std::min(std::min(gran, max_cells - cells), no - (base + cells));
      const int32_t lo = base, hi = base + cells + g;  // the tile with the granule: owned cells [lo, hi)
      ++attempt;
      int32_t newrec = 0;
      r1new.clear();
      for (int32_t o = base + cells; o < hi; ++o) {
        for (int32_t sl = 0; sl < S; ++sl) {
          const int64_t idx = (int64_t)sl * stride + o;
          const int32_t id  = nbr[idx];
          if (id == NBR_EMPTY) continue;
          const int32_t p = pos[idx];
          if (emark[p] != stamp && etry[p] != attempt) {
            etry[p] = attempt;
            ++newrec;
          }
          if (id < 0) continue;  // boundary edge: no cell beyond it
          const int32_t n  = id & NBR_MASK;
          const int32_t on = mesh->cell_is_owned[n] ? mesh->cell_local_to_owned[n] : -1;
          if (on >= lo && on < hi) continue;  // inside the tile
          if (r1mark[n] != stamp && r1try[n] != attempt) {
            r1try[n] = attempt;
            r1new.push_back(n);
          }
        }
      }
      // first-ring cells the granule swallows
      int32_t left = 0;
      for (int32_t o = base + cells; o < hi; ++o)
        if (r1mark[L.o2l[o]] == stamp) ++left;
      const int32_t nh = (int32_t)r1.size() - left + (int32_t)r1new.size();
      bool bad = rec + newrec > max_rec || nh > max_h1;
      if (!bad && L.muscl_on) {
        // second ring: the other neighbours of the (owned) first-ring cells
        int32_t n2 = 0;
        auto ring2_of = [&](int32_t cell) {
          if (!mesh->cell_is_owned[cell]) return;  // a ghost's stencil is on another rank
          const int32_t ob = mesh->cell_local_to_owned[cell];
          if (ob >= lo && ob < hi) return;          // swallowed by the granule
          for (int32_t sl = 0; sl < S; ++sl) {
            const int32_t id = nbr[(int64_t)sl * stride + ob];
            if (id < 0) continue;
            const int32_t n  = id & NBR_MASK;
            const int32_t on = mesh->cell_is_owned[n] ? mesh->cell_local_to_owned[n] : -1;
            if (on >= lo && on < hi) continue;
            if ((r1mark[n] == stamp) || r1try[n] == attempt || r2try[n] == attempt) continue;
            r2try[n] = attempt;
            ++n2;
          }
        };
        for (int32_t cell : r1) ring2_of(cell);
        for (int32_t cell : r1new) ring2_of(cell);
        // (a first-ring cell the granule swallows may still be counted as somebody's second-ring neighbour: it is inside
        // the tile then, and the test above skips it)
        bad = nh + n2 > max_ring;
      }
      if (bad) {
        if (cells > 0) break;        // the granule starts the next tile
        if (gran > 1) {              // not even one granule fits: cell by cell
          gran = 1;
          continue;
        }
        // a single cell always fits (S records, S halo cells, 3 S ring cells)
      }
      // accept
      for (int32_t o = base + cells; o < hi; ++o)
        for (int32_t sl = 0; sl < S; ++sl) {
          const int64_t idx = (int64_t)sl * stride + o;
          if (nbr[idx] != NBR_EMPTY) emark[pos[idx]] = stamp;
        }
      if (left > 0) {
        size_t w = 0;
        for (size_t i = 0; i < r1.size(); ++i) {
          const int32_t cell = r1[i];
          const int32_t on   = mesh->cell_is_owned[cell] ? mesh->cell_local_to_owned[cell] : -1;
          if (on >= lo && on < hi) r1mark[cell] = -1;
          else r1[w++] = cell;
        }
        r1.resize(w);
      }
      for (int32_t cell : r1new) {
        r1mark[cell] = stamp;
        r1.push_back(cell);
      }
      cells += g;
      rec += newrec;
    }
    base += cells;
  }
  c0.push_back(no);
  return c0;
}

// the tiles: edge records, halo-cell lists, boundary lists, slot references, and for the second-order kernel the
// first-ring stencils and the second ring
static int layout_build_tiles(const RDyHipConfig *config, const RDyHipMesh *mesh, HostLayout &L) {
  const int32_t nc = L.nc, no = L.no, ni = L.ni, S = L.S;
  const int64_t stride   = L.stride;
  const bool    muscl_on = L.muscl_on;
  const auto &nbr = L.nbr; const auto &pos = L.pos; const auto &bedge = L.bedge; const auto &bleft = L.bleft;
  (void)config;
  int32_t max_cells = TILE;
  if (const char *e = getenv("RDYHIP_TILE_CELLS")) {  // measurement knob: the largest tile
    if (atoi(e) > 0) max_cells = std::min<int32_t>(atoi(e), TILE);
  }
  std::vector<int32_t>  tile_c0 = layout_cut_tiles(mesh, L, max_cells);
  const int32_t         ntiles = (int32_t)tile_c0.size() - 1;
  std::vector<TileDesc> tiles((size_t)ntiles + 1);
  std::vector<uint32_t> e_lr;
  std::vector<int32_t>  hcells, tile_bk, tile_boff((size_t)ntiles + 1, 0), halo_tiles, e_pos;
  std::vector<double>   e_cs, e_mid;
  std::vector<int32_t>  hslot2, touched2, hcells2, c_off;
  std::vector<uint16_t> bn_idx;
  int32_t               hmax2 = 0;
  std::vector<uint16_t> slot_ref((size_t)no * 4, SLOT_EMPTY);
  int32_t               emax = 0, hmax = 0;
  {
    e_lr.reserve((size_t)no * 2);
    e_cs.reserve((size_t)no * 2);
    std::vector<std::pair<int32_t, int32_t>> items;  // (loop position of the edge, owned cell * 4 + slot)
    items.reserve(4 * TILE);
    std::vector<int32_t> hslot((size_t)nc, -1);      // local cell -> halo slot in the current tile
    std::vector<int32_t> touched;
    if (muscl_on) {
      hslot2.assign((size_t)nc, -1);
      c_off.assign((size_t)ntiles + 1, 0);
    }
    for (int32_t t = 0; t < ntiles; ++t) {
      const int32_t base = tile_c0[t], cntc = tile_c0[t + 1] - base;
      items.clear();
      bool halo_tile = false;
      for (int32_t j = 0; j < cntc; ++j) {
        for (int32_t sl = 0; sl < S; ++sl) {
          const int64_t idx = (int64_t)sl * stride + base + j;
          if (nbr[idx] == NBR_EMPTY) continue;
          items.emplace_back(pos[idx], (base + j) * 4 + sl);
          if (nbr[idx] >= 0 && (nbr[idx] & NBR_GHOST)) halo_tile = true;
        }
      }
      std::sort(items.begin(), items.end());
      tiles[t].e_off = (int32_t)e_lr.size();
      tiles[t].h_off = (int32_t)hcells.size();
      tiles[t].c_off = base;
      tile_boff[t]   = (int32_t)tile_bk.size();
      tiles[t].cnt   = halo_tile ? TILE_HALO_FLAG : 0u;   // the counts are filled in below
      if (halo_tile) halo_tiles.push_back(t);
      touched.clear();
      int32_t nh = 0, nbk = 0;
      // LDS slot of a cell: 0..255 inside the tile, 256.. for the tile's halo cells
      auto slot_of = [&](int32_t cell) -> uint32_t {
        if (mesh->cell_is_owned[cell]) {
          const int32_t oo = mesh->cell_local_to_owned[cell];
          if (oo >= base && oo < base + cntc) return (uint32_t)(oo - base);
        }
        if (hslot[cell] < 0) {
          hslot[cell] = nh++;
          hcells.push_back(cell);
          touched.push_back(cell);
        }
        return (uint32_t)(TILE + hslot[cell]);
      };
      int32_t last = -1, local = -1;
      for (const auto &it : items) {
        if (it.first != last) {
          last = it.first;
          ++local;
          int32_t  e;
          uint32_t lr;
          if (last < ni) {
            e  = mesh->edge_internal_ids[last];
            lr = slot_of(mesh->edge_cell_ids[2 * e]) | (slot_of(mesh->edge_cell_ids[2 * e + 1]) << EDGE_R_SHIFT);
            if (muscl_on && mesh->edge_is_owned && !mesh->edge_is_owned[e]) lr |= EDGE_NOT_OWNED;
            if (muscl_on) {
              // the edge midpoint of ReconstructFaceValues (src/operator_fluxes_ceed.c:1169-1172); the kernel subtracts the
              // two cell centroids itself (1175-1178)
              const int32_t v0 = mesh->edge_vertex_ids[2 * e], v1 = mesh->edge_vertex_ids[2 * e + 1];
              if (v0 < 0 || v1 < 0 || v0 >= mesh->num_vertices || v1 >= mesh->num_vertices)
                return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "edge %d has vertex ids (%d,%d) out of range", e, v0, v1);
              e_mid.push_back(0.5 * (mesh->vertex_points[3 * (size_t)v0 + 0] + mesh->vertex_points[3 * (size_t)v1 + 0]));
              e_mid.push_back(0.5 * (mesh->vertex_points[3 * (size_t)v0 + 1] + mesh->vertex_points[3 * (size_t)v1 + 1]));
            }
          } else {
            if (muscl_on) e_mid.insert(e_mid.end(), 2, 0.0);
            const int32_t k = last - ni;
            e               = bedge[k];
            lr              = slot_of(bleft[k]) | ((uint32_t)nbk << EDGE_R_SHIFT) | EDGE_BOUNDARY;
            tile_bk.push_back(k);
            ++nbk;
          }
          // unit normal as one double: the smaller-magnitude component, the other is +-sqrt(1 - cs^2)
          const double ecn = mesh->edge_cn[e], esn = mesh->edge_sn[e];
          if (std::fabs(ecn) <= std::fabs(esn)) {
            lr |= EDGE_CS_IS_CN | (std::signbit(esn) ? EDGE_OTHER_NEG : 0u);
            e_cs.push_back(ecn);
          } else {
            lr |= (std::signbit(ecn) ? EDGE_OTHER_NEG : 0u);
            e_cs.push_back(esn);
          }
          e_lr.push_back(lr);
          e_pos.push_back(last);  // records of a tile are in loop order; across tiles only this table orders them
        }
        slot_ref[(size_t)(it.second >> 2) * 4 + (it.second & 3)] = (uint16_t)local;
      }
      int32_t nc2 = 0;
      if (muscl_on) {
        // fused second-order kernel: the stencil of every first-ring cell (LDS slots of its neighbours) and the tile's
        // second ring (neighbours of first-ring cells outside tile + ring 1)
        c_off[t]    = (int32_t)hcells2.size();
        touched2.clear();
        for (int32_t b = 0; b < nh; ++b) {
          const int32_t cell  = hcells[(size_t)tiles[t].h_off + b];
          uint16_t      ix[4] = {BN_NONE, BN_NONE, BN_NONE, BN_NONE};
          if (!mesh->cell_is_owned[cell]) {
            ix[0] = ix[1] = ix[2] = ix[3] = BN_GLOBAL;  // a ghost: its stencil is on another rank
          } else {
            const int32_t ob = mesh->cell_local_to_owned[cell];
            for (int32_t sl = 0; sl < S; ++sl) {
              const int64_t idx = (int64_t)sl * stride + ob;
              const int32_t id  = nbr[idx];
              if (id < 0) continue;
              const int32_t n = id & NBR_MASK;
              if (id & NBR_GHOST) halo_tile = true;  // the tile needs a ghost's state
              int32_t slot;
              const int32_t on = mesh->cell_is_owned[n] ? mesh->cell_local_to_owned[n] : -1;
              if (on >= base && on < base + cntc) slot = on - base;
              else if (hslot[n] >= 0) slot = TILE + hslot[n];
              else {
                if (hslot2[n] < 0) {
                  hslot2[n] = nc2++;
                  hcells2.push_back(n);
                  touched2.push_back(n);
                }
                slot = TILE + nh + hslot2[n];
              }
              ix[sl] = (uint16_t)slot;
            }
          }
          bn_idx.insert(bn_idx.end(), ix, ix + 4);
        }
        for (int32_t cell : touched2) hslot2[cell] = -1;
        hmax2 = std::max(hmax2, nh + nc2);
        tiles[t].cnt = halo_tile ? TILE_HALO_FLAG : 0u;
        if (halo_tile && (halo_tiles.empty() || halo_tiles.back() != t)) halo_tiles.push_back(t);
      }
      for (int32_t cell : touched) hslot[cell] = -1;
      // what layout_cut_tiles promised (the kernels' LDS planes and register rounds have exactly this room)
      const int32_t cap_h1 = S == 3 ? TILE_MAX_HALO_TRI : TILE_MAX_HALO_QUAD, cap_ring = S == 3 ? MUSCL_MAX_RING_TRI : MUSCL_MAX_RING_QUAD;
      if (cntc < 1 || cntc > TILE || local + 1 > TILE_MAX_REC || nh > cap_h1 || (muscl_on && nh + nc2 > cap_ring))
        return fail(RDYHIP_ERR_LIB, "internal error: tile %d (%d cells, %d edge records, %d + %d ring cells) exceeds the kernels' capacities", t, cntc, local + 1, nh, nc2);
      tiles[t].cnt |= (uint32_t)(local + 1) | ((uint32_t)nh << 11) | ((uint32_t)(cntc - 1) << 22);
      emax = std::max(emax, local + 1);
      hmax = std::max(hmax, nh);
      if ((int64_t)e_lr.size() > (int64_t)INT32_MAX - 4 * TILE) return fail(RDYHIP_ERR_ARG_SIZ, "too many tile edge records");
    }
    tiles[ntiles].e_off = (int32_t)e_lr.size();
    tiles[ntiles].h_off = (int32_t)hcells.size();
    tiles[ntiles].c_off = no;
    tile_boff[ntiles]   = (int32_t)tile_bk.size();
    tiles[ntiles].cnt   = 0;
    if (muscl_on) c_off[ntiles] = (int32_t)hcells2.size();
  }
  L.ntiles = ntiles; L.emax = emax; L.hmax = hmax; L.hmax2 = hmax2;
  L.hcells = std::move(hcells); L.tile_bk = std::move(tile_bk); L.tile_boff = std::move(tile_boff); L.halo_tiles = std::move(halo_tiles);
  L.hcells2 = std::move(hcells2); L.tile_c0 = std::move(tile_c0);
  L.c_off = std::move(c_off); L.e_cs = std::move(e_cs); L.e_mid = std::move(e_mid); L.tiles = std::move(tiles);
  // ---- extra Courant edges: the reference's interior loop covers every local internal edge with len / min(area_l, area_r)
  // (swe_petsc.c:275-296); the slots of the owned cells cover an edge from the owned side(s) only
  for (int32_t p = 0; p < ni; ++p) {
    const int32_t e = mesh->edge_internal_ids[p];
    const int32_t l = mesh->edge_cell_ids[2 * e], r = mesh->edge_cell_ids[2 * e + 1];
    if (r == -1) continue;
    const bool   lo = mesh->cell_is_owned[l] != 0, ro = mesh->cell_is_owned[r] != 0;
    const double al = mesh->cell_areas[l], ar = mesh->cell_areas[r];
    if (lo && ro) continue;
    if (lo != ro && !((lo ? ar : al) < (lo ? al : ar))) continue;  // the owned cell is the smaller one (or equal): its slot has len / min already
    // second order: only the rank that owns an edge reports it (swe_petsc.c:172-190) -- never an edge between two ghosts
    if (muscl_on && mesh->edge_is_owned && !mesh->edge_is_owned[e]) continue;
    if (muscl_on && !mesh->edge_is_owned && !lo && !ro) continue;
    L.x_lr.push_back(l);
    L.x_lr.push_back(r);
    L.x_pos.push_back(p);
    const double ecn = mesh->edge_cn[e], esn = mesh->edge_sn[e];
    if (std::fabs(ecn) <= std::fabs(esn)) {
      L.x_flags.push_back(EDGE_CS_IS_CN | (std::signbit(esn) ? EDGE_OTHER_NEG : 0u));
      L.x_cs.push_back(ecn);
    } else {
      L.x_flags.push_back(std::signbit(ecn) ? EDGE_OTHER_NEG : 0u);
      L.x_cs.push_back(esn);
    }
    L.x_cfac.push_back(mesh->edge_lengths[e] / std::min(al, ar));
    if (muscl_on) {
      const int32_t v0 = mesh->edge_vertex_ids[2 * e], v1 = mesh->edge_vertex_ids[2 * e + 1];
      if (v0 < 0 || v1 < 0 || v0 >= mesh->num_vertices || v1 >= mesh->num_vertices)
        return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "edge %d has vertex ids (%d,%d) out of range", e, v0, v1);
      L.x_mid.push_back(0.5 * (mesh->vertex_points[3 * (size_t)v0 + 0] + mesh->vertex_points[3 * (size_t)v1 + 0]));
      L.x_mid.push_back(0.5 * (mesh->vertex_points[3 * (size_t)v0 + 1] + mesh->vertex_points[3 * (size_t)v1 + 1]));
    }
  }
  L.e_pos = std::move(e_pos);
  L.e_pos.insert(L.e_pos.end(), L.x_pos.begin(), L.x_pos.end());  // extra edge i is "record" nrec + i
  L.e_lr = std::move(e_lr); L.slot_ref = std::move(slot_ref); L.bn_idx = std::move(bn_idx);
  return 0;
}

static int build_host_layout(const RDyHipConfig *config, const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries,
                             HostLayout &L) {
  int rc = layout_check_arguments(config, mesh, num_boundaries, boundaries);
  if (!rc) rc = layout_build_slots(config, mesh, num_boundaries, boundaries, L);
  if (!rc) rc = layout_build_tiles(config, mesh, L);
  if (rc) return rc;
  const int32_t no = L.no;
  const auto   &o2l      = L.o2l;
  const bool   hr_on     = config->well_balancing == RDYHIP_WELL_BALANCING_HR;
  const size_t lds_bytes = tiled_lds_bytes(L.S, hr_on);
  const size_t lds_muscl = !L.muscl_on ? 0 : muscl_lds_bytes(L.S);
  static_assert(tiled_lds_bytes(4, true) <= 64 * 1024 && muscl_lds_bytes(3) <= 64 * 1024 && muscl_lds_bytes(4) <= 64 * 1024,
                "the kernels' LDS fits the default dynamic allocation");

  // ---- per-owned-cell geometry --------------------------------------------
  std::vector<double> dzdx((size_t)no), dzdy((size_t)no);
  for (int32_t o = 0; o < no; ++o) {
    dzdx[o] = mesh->cell_dz_dx[o2l[o]];
    dzdy[o] = mesh->cell_dz_dy[o2l[o]];
  }

  L.hr_on = hr_on; L.lds_bytes = lds_bytes; L.lds_muscl = lds_muscl;
  L.dzdx = std::move(dzdx); L.dzdy = std::move(dzdy);
  const int32_t nc = L.nc;
  if (L.S == 3) {
    L.ref3.resize((size_t)no);
    for (int32_t o = 0; o < no; ++o) {
      uint32_t w = 0;
      for (int sl = 0; sl < 3; ++sl) {
        const uint16_t r = L.slot_ref[(size_t)o * 4 + sl];
        w |= (r == SLOT_EMPTY ? REF3_EMPTY : (uint32_t)r) << (10 * sl);
      }
      L.ref3[o] = w;
    }
  }
  if (hr_on) L.zc.assign(mesh->cell_zc, mesh->cell_zc + nc);
  if (L.muscl_on) {
    L.cxy.resize((size_t)2 * nc);
    for (int32_t c = 0; c < nc; ++c) {
      L.cxy[2 * (size_t)c]     = mesh->cell_centroids[3 * (size_t)c + 0];
      L.cxy[2 * (size_t)c + 1] = mesh->cell_centroids[3 * (size_t)c + 1];
    }
  }
  LayoutCounts &n = L.counts;
  n.n_cells = nc; n.n_owned = no; n.S = L.S; n.K = L.K; n.n_halo = (int32_t)L.halo.size(); n.ntiles = L.ntiles;
  n.n_halo_tiles = (int32_t)L.halo_tiles.size(); n.emax = L.emax; n.hmax = L.hmax; n.hmax2 = L.hmax2;
  n.nrec = (int64_t)L.e_lr.size(); n.nhalo_entries = (int64_t)L.hcells.size(); n.n_hcells2 = (int64_t)L.hcells2.size();
  n.prefix = L.prefix; n.muscl = L.muscl_on; n.lds_bytes = lds_bytes; n.lds_muscl = lds_muscl;
  return 0;
}

// rdyhip_layout_info (the operator's launch choices and device memory) and rdyhip_probe_layout (tiled kernel, no device)
static void fill_layout_info(const LayoutCounts &n, bool use_tiled, int persistent_grid, int64_t device_bytes, RDyHipLayoutInfo *info) {
  info->num_owned_cells    = n.n_owned;
  info->num_cells          = n.n_cells;
  info->slots_per_cell     = n.S;
  info->num_boundary_edges = n.K;
  info->num_halo_cells     = n.n_halo;
  info->tiled_kernel       = use_tiled ? 1 : 0;
  info->num_tiles          = n.ntiles;
  info->num_halo_tiles     = n.n_halo_tiles;
  info->max_tile_edges     = n.emax;
  info->max_tile_halo_cells = n.hmax;
  info->num_halo_entries   = n.nhalo_entries;
  info->num_edge_records   = n.nrec;
  info->owned_is_prefix    = n.prefix ? 1 : 0;
  info->device_bytes       = device_bytes;
  info->second_order_fused   = n.muscl ? 1 : 0;
  info->max_tile_ring2_cells = n.hmax2;
  info->persistent_grid      = persistent_grid;
  info->lds_bytes            = (int32_t)(n.muscl ? n.lds_muscl : n.lds_bytes);
  info->lds_fixed_layout     = use_tiled ? 1 : 0;  // every tile is cut to the kernels' fixed LDS capacities
  // u (own cell) 24 + slots S*(4+8+8+8) + dz 16 + n 8 + ext src 24 + F 24 + pv 24 (+4 for o2l)
  if (use_tiled) {
    // u 24 + slot refs 4 (8 for quads) + coef S*8 + dz 16 + n 8 + ext src 24 + F 24 + pv 24 (+4 for o2l) per cell;
    // 12 B per edge record; 4 B id per halo-cell entry (the halo states themselves are mostly L2 hits)
    info->bytes_per_apply = (int64_t)n.n_owned * (24 + (n.S == 3 ? 4 : 8) + n.S * 8 + 16 + 8 + 24 + 24 + 24 + (n.prefix ? 0 : 4)) +
                            n.nrec * 12 + n.nhalo_entries * 4 + (int64_t)n.ntiles * 16;
  } else {
    info->bytes_per_apply = (int64_t)n.n_owned * (24 + n.S * 28 + 16 + 8 + 24 + 24 + 24 + (n.prefix ? 0 : 4));
  }
  if (n.muscl) {
    // + the cell centroid (16 B per cell) and the edge midpoint (16 B per edge record); fused: second-ring ids and the
    // first-ring stencils (8 B per halo entry); split: the gradient array written and read (96) + the state, the centroid and
    // the neighbour ids read a second time (24 + 16 + S*4)
    info->bytes_per_apply += (int64_t)n.n_owned * 16 + n.nrec * 16;
    info->bytes_per_apply += n.n_hcells2 * 4 + n.nhalo_entries * 8;
  }
}

}  // namespace rdyhip
