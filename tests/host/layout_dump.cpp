// Stand-alone host program around the layout pass (rdycore_amd/csrc/host_layout.h): reads one mesh from a flat binary file
// (written by tests/test_layout_tables_cpu.py), runs build_host_layout and prints, as one JSON object, the RDyHipLayoutInfo
// numbers and a 64-bit FNV-1a hash of the bytes of every table of HostLayout.  Built with the host compiler under the address
// and undefined-behaviour sanitizers; every input array is a heap block of exactly the caller's length, so that a read past
// an array's end is a report.  A layout error: {"rc": code, "error": message} and the code as the exit status.
//
// File: "RDYLAY01" | RDyHipConfig | int32 num_cells, num_owned_cells, num_edges, num_internal_edges, num_vertices,
// num_boundaries | the 17 arrays of RDyHipMesh in its declaration order, each int64 count (-1: null pointer) + data |
// per boundary int32 condition_type, int64 count (-1: null) + int32 edge ids.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>

#include "host_layout.h"

using namespace rdyhip;

namespace {

struct Reader {
  FILE *f;
  std::vector<std::unique_ptr<char[]>> blocks;
  void raw(void *dst, size_t n) {
    if (n && fread(dst, 1, n, f) != n) {
      fprintf(stdout, "{\"rc\": -1, \"error\": \"short input file\"}\n");
      exit(2);
    }
  }
  template <class T>
  T scalar() {
    T v;
    raw(&v, sizeof(T));
    return v;
  }
  template <class T>
  const T *array(int64_t *count = nullptr) {
    const int64_t n = scalar<int64_t>();
    if (count) *count = std::max<int64_t>(n, 0);
    if (n < 0) return nullptr;
    blocks.emplace_back(new char[(size_t)n * sizeof(T)]);   // exactly n elements (n == 0: a valid, empty block)
    raw(blocks.back().get(), (size_t)n * sizeof(T));
    return reinterpret_cast<const T *>(blocks.back().get());
  }
};

template <class T>
uint64_t fnv1a(const std::vector<T> &v) {
  uint64_t             h = 0xcbf29ce484222325ull;
  const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  Reader r{fopen(argv[1], "rb"), {}};
  if (!r.f) return 2;
  char magic[8];
  r.raw(magic, 8);
  if (memcmp(magic, "RDYLAY01", 8) != 0) return 2;
  const RDyHipConfig config = r.scalar<RDyHipConfig>();
  RDyHipMesh         m{};
  m.num_cells          = r.scalar<int32_t>();
  m.num_owned_cells    = r.scalar<int32_t>();
  m.num_edges          = r.scalar<int32_t>();
  m.num_internal_edges = r.scalar<int32_t>();
  m.num_vertices       = r.scalar<int32_t>();
  const int32_t nb     = r.scalar<int32_t>();
  m.cell_is_owned       = r.array<int32_t>();
  m.cell_local_to_owned = r.array<int32_t>();
  m.cell_global_ids     = r.array<int64_t>();
  m.cell_areas          = r.array<double>();
  m.cell_dz_dx          = r.array<double>();
  m.cell_dz_dy          = r.array<double>();
  m.edge_cell_ids       = r.array<int32_t>();
  m.edge_internal_ids   = r.array<int32_t>();
  m.edge_global_ids     = r.array<int64_t>();
  m.edge_lengths        = r.array<double>();
  m.edge_cn             = r.array<double>();
  m.edge_sn             = r.array<double>();
  m.cell_zc             = r.array<double>();
  m.cell_centroids      = r.array<double>();
  m.edge_vertex_ids     = r.array<int32_t>();
  m.vertex_points       = r.array<double>();
  m.edge_is_owned       = r.array<int32_t>();
  std::vector<RDyHipBoundary> b((size_t)std::max(nb, 0));
  for (auto &x : b) {
    x.condition_type = r.scalar<int32_t>();
    int64_t n        = 0;
    x.edge_ids       = r.array<int32_t>(&n);
    x.num_edges      = (int32_t)n;
  }
  fclose(r.f);

  HostLayout L;
  const int  rc = build_host_layout(&config, &m, nb, b.data(), L);
  if (rc) {
    printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, g_err.c_str());   // (no message of the layout pass holds a quote or a backslash)
    return rc;
  }
  RDyHipLayoutInfo i{};
  fill_layout_info(L.counts, true, 0, 0, &i);
  printf("{\"rc\": 0, \"info\": {\"num_owned_cells\": %d, \"num_cells\": %d, \"slots_per_cell\": %d, \"num_boundary_edges\": %d, "
         "\"num_halo_cells\": %d, \"tiled_kernel\": %d, \"num_tiles\": %d, \"num_halo_tiles\": %d, \"max_tile_edges\": %d, "
         "\"max_tile_halo_cells\": %d, \"num_halo_entries\": %" PRId64 ", \"num_edge_records\": %" PRId64 ", \"owned_is_prefix\": %d, "
         "\"device_bytes\": %" PRId64 ", \"bytes_per_apply\": %" PRId64 ", \"second_order_fused\": %d, \"max_tile_ring2_cells\": %d, "
         "\"persistent_grid\": %d, \"lds_bytes\": %d, \"lds_fixed_layout\": %d},\n \"tables\": {",
         i.num_owned_cells, i.num_cells, i.slots_per_cell, i.num_boundary_edges, i.num_halo_cells, i.tiled_kernel, i.num_tiles, i.num_halo_tiles,
         i.max_tile_edges, i.max_tile_halo_cells, i.num_halo_entries, i.num_edge_records, i.owned_is_prefix, i.device_bytes, i.bytes_per_apply,
         i.second_order_fused, i.max_tile_ring2_cells, i.persistent_grid, i.lds_bytes, i.lds_fixed_layout);
  const char *sep = "";
#define TABLE(name)                                                        \
  printf("%s\"" #name "\": \"%016" PRIx64 "\"", sep, fnv1a(L.name)); \
  sep = ", "
  // the vectors of HostLayout in their declared order
  TABLE(o2l); TABLE(boff); TABLE(nbr); TABLE(pos); TABLE(btype); TABLE(bleft); TABLE(bedge); TABLE(bghost); TABLE(halo); TABLE(hcells);
  TABLE(tile_bk); TABLE(tile_boff); TABLE(tile_c0); TABLE(halo_tiles); TABLE(hcells2); TABLE(c_off); TABLE(e_pos);
  TABLE(cn); TABLE(sn); TABLE(coef); TABLE(bcn); TABLE(bsn); TABLE(e_cs); TABLE(e_mid); TABLE(dzdx); TABLE(dzdy);
  TABLE(tiles); TABLE(e_lr); TABLE(x_lr); TABLE(x_pos); TABLE(x_flags); TABLE(x_cs); TABLE(x_cfac); TABLE(x_mid);
  TABLE(slot_ref); TABLE(bn_idx); TABLE(ref3); TABLE(cxy); TABLE(zc);
#undef TABLE
  printf("}}\n");
  return 0;
}
