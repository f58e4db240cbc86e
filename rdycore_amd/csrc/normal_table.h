// The normal table: the host-side pass that turns the per-record edge normals of a finished layout into a table of the
// distinct ones, where there are few.  No HIP, no operator: plain C++17 over the e_lr / e_cs tables of host_layout.h, so the
// pass can be tested on the host (tests/test_normal_table_cpu.py).  Included by rdyhip_api.hip.
//
// A record's normal is the triple (stored component, EDGE_CS_IS_CN, EDGE_OTHER_NEG) (tile_format.h).  The KEY of a record is
// that triple with the component taken as its 64-bit pattern: -0.0 is not +0.0, so that the table kernel gives edge_normal
// the very operands the streamed kernel gives it.  The edges of a raster-derived mesh -- axis-parallel sides and one or two
// diagonals, in both orientations -- have six or eight keys whatever the mesh's size; an unstructured mesh has about as many as
// it has edges.  With at most NORMAL_TABLE_MAX keys, each record's word gets the index of its key in bits 26-31
// (EDGE_NT_SHIFT), which no reader of the word looks at but the table kernels; bits 0-25 stay what they were.
#pragma once
#include <stdint.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "tile_format.h"

namespace rdyhip {

struct NormalTable {
  bool                  active = false;  // the words carry indices and `cs` / `flags` are the entries
  std::vector<double>   cs;              // stored component of each entry, in order of first appearance
  std::vector<uint32_t> flags;           // its EDGE_CS_IS_CN | EDGE_OTHER_NEG bits, where a record's word has them
};

// e_lr[i] / e_cs[i]: the n records.  Returns the table; active only if n > 0 and the records have <= NORMAL_TABLE_MAX keys,
// and only then are the words changed (an index OR-ed into bits 26-31, which must be clear on entry: they are, in every
// word build_host_layout writes -- a word that has one set makes the pass report "streamed" and leaves all words alone).
inline NormalTable build_normal_table(uint32_t *e_lr, const double *e_cs, size_t n) {
  NormalTable t;
  if (n == 0 || !e_lr || !e_cs) return t;
  constexpr uint32_t HIGH = ~((1u << EDGE_NT_SHIFT) - 1u);
  struct Key {
    uint64_t bits;
    uint32_t flags;
    bool     operator==(const Key &o) const { return bits == o.bits && flags == o.flags; }
  };
  struct KeyHash {
    size_t operator()(const Key &k) const { return (size_t)((k.bits ^ (k.bits >> 29)) * 0x9E3779B97F4A7C15ull + k.flags); }
  };
  std::unordered_map<Key, uint8_t, KeyHash> index;
  std::vector<uint8_t>                      of_record(n);
  for (size_t i = 0; i < n; ++i) {
    if (e_lr[i] & HIGH) return NormalTable{};
    Key k;
    memcpy(&k.bits, e_cs + i, sizeof(k.bits));
    k.flags       = e_lr[i] & EDGE_NT_FLAGS;
    const auto it = index.find(k);
    if (it != index.end()) {
      of_record[i] = it->second;
      continue;
    }
    if (t.cs.size() == (size_t)NORMAL_TABLE_MAX) return NormalTable{};  // one key too many: streamed, nothing was written
    of_record[i] = (uint8_t)t.cs.size();
    index.emplace(k, of_record[i]);
    t.cs.push_back(e_cs[i]);
    t.flags.push_back(k.flags);
  }
  for (size_t i = 0; i < n; ++i) e_lr[i] |= (uint32_t)of_record[i] << EDGE_NT_SHIFT;
  t.active = true;
  return t;
}

}  // namespace rdyhip
