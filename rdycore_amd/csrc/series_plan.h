// The record plan of the boundary-flux time series (rdyhip_series_*): which boundary edges a record holds and in what order.
// It restates the loops of RecordBoundaryFluxes / WriteBoundaryFluxes (src/time_series.c:270-335):
//   for every boundary b in ascending index that is listed (the reference: whose condition is not auto-generated)
//     for every edge e of b in edge_ids order
//       if the edge's left cell edges.cell_ids[2 * e] is owned: the next row of the record
// so slot[k] -- k counts the boundary edges of all boundaries concatenated, the rows of boundary_fluxes_accum -- is the row
// of edge k in a record, or -1 for an edge of an unlisted boundary or behind a ghost cell.
// No device call anywhere in this file, and no HIP header: like host_layout.h it includes only rdyhip.h, error.h and the
// standard library and builds with a plain host compiler into a stand-alone program (tests/host/series_plan_dump.cpp, run
// under the address and undefined-behaviour sanitizers by tests/test_series_cpu.py).
#pragma once
#include <cstdint>
#include <vector>

#include "rdyhip.h"
#include "error.h"

namespace rdyhip {

struct SeriesPlan {
  std::vector<int32_t> slot;      // [K] row in a record, or -1
  std::vector<int32_t> edge;      // [E] local edge id of each recorded edge
  std::vector<int32_t> boundary;  // [E] the boundary it belongs to
  std::vector<double>  len;       // [K] edges.lengths of every boundary edge
  int32_t              E = 0;
};

// listed[0 .. num_listed) -> one flag per boundary; listed == nullptr: every boundary.  A boundary named twice counts once.
static int series_listed_mask(int32_t num_boundaries, int32_t num_listed, const int32_t *listed, std::vector<uint8_t> &mask) {
  if (num_boundaries < 0) return fail(RDYHIP_ERR_USER, "bad boundary list");
  mask.assign((size_t)num_boundaries, listed ? 0 : 1);
  if (!listed) return 0;
  if (num_listed < 0) return fail(RDYHIP_ERR_USER, "negative number of listed boundaries (%d)", num_listed);
  for (int32_t i = 0; i < num_listed; ++i) {
    if (listed[i] < 0 || listed[i] >= num_boundaries) return fail(RDYHIP_ERR_USER, "Invalid boundary index %d", listed[i]);
    mask[(size_t)listed[i]] = 1;
  }
  return 0;
}

// The loops above over the concatenated boundary-edge table: boff[num_boundaries + 1], bedge[K] the local edge ids,
// left_owned[k] != 0 where the left cell of boundary edge k is owned.  Fills slot, edge, boundary and E.
static void series_plan_rows(int32_t num_boundaries, const int32_t *boff, const int32_t *bedge, const uint8_t *left_owned,
                             const std::vector<uint8_t> &mask, SeriesPlan &P) {
  const int32_t K = num_boundaries > 0 ? boff[num_boundaries] : 0;
  P.slot.assign((size_t)K, -1);
  P.edge.clear();
  P.boundary.clear();
  for (int32_t b = 0; b < num_boundaries; ++b) {
    if (!mask[(size_t)b]) continue;
    for (int32_t k = boff[b]; k < boff[b + 1]; ++k) {
      if (!left_owned[k]) continue;
      P.slot[(size_t)k] = (int32_t)P.edge.size();
      P.edge.push_back(bedge[k]);
      P.boundary.push_back(b);
    }
  }
  P.E = (int32_t)P.edge.size();
}

// The plan from the caller's mesh arrays (rdyhip_series_plan_boundary_edges): validates what it reads as the layout pass does
static int series_plan_from_mesh(const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries, int32_t num_listed,
                                 const int32_t *listed, SeriesPlan &P) {
  if (!mesh) return fail(RDYHIP_ERR_USER, "null mesh");
  if (num_boundaries < 0 || (num_boundaries > 0 && !boundaries)) return fail(RDYHIP_ERR_USER, "bad boundary list");
  std::vector<uint8_t> mask;
  int                  rc = series_listed_mask(num_boundaries, num_listed, listed, mask);
  if (rc) return rc;
  const int32_t nc = mesh->num_cells, ne = mesh->num_edges;
  if (nc < 0 || ne < 0) return fail(RDYHIP_ERR_ARG_SIZ, "inconsistent mesh sizes");
  std::vector<int32_t> boff((size_t)num_boundaries + 1, 0);
  for (int32_t b = 0; b < num_boundaries; ++b) {
    if (boundaries[b].num_edges < 0 || (boundaries[b].num_edges > 0 && !boundaries[b].edge_ids)) return fail(RDYHIP_ERR_USER, "bad boundary %d", b);
    boff[(size_t)b + 1] = boff[(size_t)b] + boundaries[b].num_edges;
  }
  const int32_t K = boff[(size_t)num_boundaries];
  if (K > 0 && (!mesh->edge_cell_ids || !mesh->edge_lengths)) return fail(RDYHIP_ERR_USER, "null edge array");
  if (K > 0 && !mesh->cell_is_owned) return fail(RDYHIP_ERR_USER, "null cell array");
  std::vector<int32_t> bedge((size_t)K);
  std::vector<uint8_t> left_owned((size_t)K);
  P.len.assign((size_t)K, 0.0);
  for (int32_t b = 0; b < num_boundaries; ++b) {
    for (int32_t i = 0; i < boundaries[b].num_edges; ++i) {
      const int32_t k = boff[(size_t)b] + i, e = boundaries[b].edge_ids[i];
      if (e < 0 || e >= ne) return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "boundary %d edge id %d out of range", b, e);
      const int32_t l = mesh->edge_cell_ids[2 * (size_t)e];
      if (l < 0 || l >= nc) return fail(RDYHIP_ERR_ARG_OUTOFRANGE, "boundary edge %d has no left cell", e);
      bedge[(size_t)k]      = e;
      left_owned[(size_t)k] = mesh->cell_is_owned[l] ? 1 : 0;
      P.len[(size_t)k]      = mesh->edge_lengths[e];
    }
  }
  series_plan_rows(num_boundaries, boff.data(), bedge.data(), left_owned.data(), mask, P);
  return 0;
}

}  // namespace rdyhip
