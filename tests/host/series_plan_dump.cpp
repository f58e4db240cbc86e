// Stand-alone host program around the record plan of the boundary-flux time series (rdycore_amd/csrc/series_plan.h): reads one
// mesh from the flat binary file tests/test_layout_tables_cpu.py writes (write_case; layout_dump.cpp describes it), takes the
// listed boundaries from the command line and prints the plan as one JSON object.  Built with the host compiler under the
// address and undefined-behaviour sanitizers; every input array is a heap block of exactly the caller's length, so that a
// read past an array's end is a report.  A plan error: {"rc": code, "error": message} and the code as the exit status.
//
//   series_plan_dump case.bin all | none | b0,b1,...
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "series_plan.h"

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

void print_list(const char *name, const std::vector<int32_t> &v, const char *end) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
  printf("]%s", end);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  Reader r{fopen(argv[1], "rb"), {}};
  if (!r.f) return 2;
  char magic[8];
  r.raw(magic, 8);
  if (memcmp(magic, "RDYLAY01", 8) != 0) return 2;
  (void)r.scalar<RDyHipConfig>();
  RDyHipMesh m{};
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

  // the list: a heap block of exactly its length, or a null pointer for "all"
  std::unique_ptr<int32_t[]> listed;
  int32_t                    num_listed = 0;
  const std::string          arg        = argv[2];
  if (arg != "all") {
    std::vector<int32_t> ids;
    if (arg != "none") {
      for (size_t p = 0; p <= arg.size();) {
        const size_t q = std::min(arg.find(',', p), arg.size());
        ids.push_back(atoi(arg.substr(p, q - p).c_str()));
        p = q + 1;
      }
    }
    num_listed = (int32_t)ids.size();
    listed.reset(new int32_t[ids.size()]);
    std::copy(ids.begin(), ids.end(), listed.get());
  }

  SeriesPlan P;
  const int  rc = series_plan_from_mesh(&m, nb, b.data(), num_listed, listed.get(), P);
  if (rc) {
    printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, g_err.c_str());
    return rc;
  }
  printf("{\"rc\": 0, \"num_edges\": %d, ", P.E);
  print_list("slot", P.slot, ", ");
  print_list("edge", P.edge, ", ");
  print_list("boundary", P.boundary, ", ");
  double len_sum = 0.0;
  for (double l : P.len) len_sum += l;
  printf("\"len_sum\": %.17g}\n", len_sum);
  return 0;
}
