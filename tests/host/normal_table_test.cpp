// Stand-alone host program over rdycore_amd/csrc/normal_table.h (no HIP, no operator): the pass that turns the per-record edge
// normals into a table of the distinct ones, one "PASS <name>" / "FAIL <name>" line per check.  Built under the address and
// undefined-behaviour sanitizers and run directly by tests/test_normal_table_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "normal_table.h"

using namespace rdyhip;

static int failures = 0;
static void check(const char *name, bool ok) {
  printf("%s %s\n", ok ? "PASS" : "FAIL", name);
  if (!ok) ++failures;
}
static uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}

constexpr uint32_t LOW = (1u << EDGE_NT_SHIFT) - 1u;

// n records over `keys` distinct (cs, flags) pairs in a scrambled order, every word with other low bits of its own: slots,
// the boundary bit on some, EDGE_NOT_OWNED on some
struct Records {
  std::vector<uint32_t> lr;
  std::vector<double>   cs;
};
static Records make_records(size_t n, int keys) {
  Records r;
  for (size_t i = 0; i < n; ++i) {
    const int    k     = (int)((i * 7 + (i >> 3)) % (size_t)keys);
    const double c     = 0.001 * (double)(k / 4 + 1) * ((k & 1) ? -1.0 : 1.0);
    uint32_t     flags = ((k >> 1) & 1) ? EDGE_CS_IS_CN : 0u;
    if (k % 3 == 0) flags |= EDGE_OTHER_NEG;
    // keys differ in (|c| step, sign, CS_IS_CN): k / 4, k & 1, (k >> 1) & 1 identify k; OTHER_NEG follows k
    uint32_t w = (uint32_t)(i % 360) | ((uint32_t)((i * 13) % 360) << EDGE_R_SHIFT) | flags;
    if (i % 11 == 0) w |= EDGE_BOUNDARY;
    if (i % 17 == 0) w |= EDGE_NOT_OWNED;
    r.lr.push_back(w);
    r.cs.push_back(c);
  }
  return r;
}
// every record's entry reproduces its own (cs bits, flags); bits 0-25 are the input's
static bool table_is_consistent(const Records &in, const Records &out, const NormalTable &t) {
  if (!t.active || t.cs.size() != t.flags.size() || t.cs.size() > (size_t)NORMAL_TABLE_MAX) return false;
  for (size_t i = 0; i < in.lr.size(); ++i) {
    if ((out.lr[i] & LOW) != in.lr[i]) return false;
    const uint32_t e = out.lr[i] >> EDGE_NT_SHIFT;
    if (e >= t.cs.size()) return false;
    if (bits_of(t.cs[e]) != bits_of(in.cs[i]) || t.flags[e] != (in.lr[i] & EDGE_NT_FLAGS)) return false;
  }
  // distinct entries
  for (size_t a = 0; a < t.cs.size(); ++a)
    for (size_t b = a + 1; b < t.cs.size(); ++b)
      if (bits_of(t.cs[a]) == bits_of(t.cs[b]) && t.flags[a] == t.flags[b]) return false;
  return true;
}

static void count_case(const char *name, int keys, bool want_active) {
  const Records in  = make_records(4000, keys);
  Records       out = in;
  const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), out.lr.size());
  bool ok;
  if (want_active) ok = table_is_consistent(in, out, t) && (int)t.cs.size() == keys;
  else ok = !t.active && t.cs.empty() && t.flags.empty() && out.lr == in.lr;  // every word untouched
  check(name, ok);
}

int main() {
  static_assert(NORMAL_TABLE_MAX == 64 && EDGE_NT_SHIFT == 26, "six free bits above EDGE_NOT_OWNED");
  static_assert(((EDGE_SLOT_MASK | (EDGE_SLOT_MASK << EDGE_R_SHIFT) | EDGE_BOUNDARY | EDGE_CS_IS_CN | EDGE_OTHER_NEG | EDGE_NOT_OWNED) & ~LOW) == 0,
                "every field of a word lies below the index");
  {
    uint32_t w = 5;
    double   c = 0.25;
    check("no_records", !build_normal_table(nullptr, nullptr, 0).active && !build_normal_table(&w, &c, 0).active && w == 5);
  }
  count_case("keys_1", 1, true);
  count_case("keys_6", 6, true);
  count_case("keys_64", 64, true);
  count_case("keys_65_is_streamed_and_untouched", 65, false);
  count_case("keys_200_is_streamed_and_untouched", 200, false);
  {  // the 65th key appears in the very last record: nothing may have been written before the pass knew
    Records in = make_records(4000, 64);
    in.cs.back() = 0.5;
    Records       out = in;
    const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), out.lr.size());
    check("late_65th_key_leaves_every_word_untouched", !t.active && out.lr == in.lr);
  }
  {  // order of first appearance
    Records in;
    const double   c[5] = {0.3, -0.3, 0.3, 0.0, -0.3};
    const uint32_t f[5] = {0, 0, EDGE_CS_IS_CN, 0, 0};
    for (int i = 0; i < 5; ++i) in.lr.push_back((uint32_t)i | f[i]), in.cs.push_back(c[i]);
    Records       out = in;
    const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), 5);
    check("entries_in_order_of_first_appearance",
          table_is_consistent(in, out, t) && t.cs.size() == 4 && t.cs[0] == 0.3 && t.cs[1] == -0.3 && t.cs[2] == 0.3 && t.flags[2] == EDGE_CS_IS_CN &&
              (out.lr[4] >> EDGE_NT_SHIFT) == 1 && (out.lr[0] >> EDGE_NT_SHIFT) == 0);
  }
  {  // +0.0 and -0.0 are different keys (an axis-parallel edge stores one or the other)
    Records in;
    for (int i = 0; i < 40; ++i) in.lr.push_back((uint32_t)i | EDGE_CS_IS_CN), in.cs.push_back((i & 1) ? -0.0 : 0.0);
    Records       out = in;
    const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), in.lr.size());
    check("plus_and_minus_zero_are_two_keys", table_is_consistent(in, out, t) && t.cs.size() == 2 && !std::signbit(t.cs[0]) && std::signbit(t.cs[1]));
  }
  {  // equal cs, different flag bits: four keys
    Records in;
    const uint32_t f[4] = {0, EDGE_CS_IS_CN, EDGE_OTHER_NEG, EDGE_CS_IS_CN | EDGE_OTHER_NEG};
    for (int i = 0; i < 64; ++i) in.lr.push_back(((uint32_t)i << EDGE_R_SHIFT) | f[i & 3]), in.cs.push_back(0.125);
    Records       out = in;
    const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), in.lr.size());
    check("equal_cs_with_different_flags_are_different_keys", table_is_consistent(in, out, t) && t.cs.size() == 4);
  }
  {  // bits that are no part of the key do not split one: boundary records, not-owned records, any slots
    Records in;
    for (int i = 0; i < 300; ++i) {
      uint32_t w = (uint32_t)i | ((uint32_t)(359 - i) << EDGE_R_SHIFT) | EDGE_OTHER_NEG;
      if (i % 2) w |= EDGE_BOUNDARY;
      if (i % 5 == 0) w |= EDGE_NOT_OWNED;
      in.lr.push_back(w);
      in.cs.push_back(-0.6);
    }
    Records       out = in;
    const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), in.lr.size());
    check("boundary_records_share_the_keys", table_is_consistent(in, out, t) && t.cs.size() == 1);
  }
  {  // a word that already has a high bit set: the pass does not guess, it streams
    Records in = make_records(100, 6);
    in.lr[57] |= 1u << 29;
    Records       out = in;
    const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), in.lr.size());
    check("occupied_high_bits_mean_streamed", !t.active && out.lr == in.lr);
  }
  {  // NaN payloads are patterns like any other
    Records in;
    double  nan_a, nan_b;
    const uint64_t a = 0x7ff8000000000001ull, b = 0x7ff8000000000002ull;
    memcpy(&nan_a, &a, 8);
    memcpy(&nan_b, &b, 8);
    for (int i = 0; i < 10; ++i) in.lr.push_back((uint32_t)i), in.cs.push_back((i & 1) ? nan_a : nan_b);
    Records       out = in;
    const NormalTable t = build_normal_table(out.lr.data(), out.cs.data(), in.lr.size());
    check("nan_payloads_are_patterns", table_is_consistent(in, out, t) && t.cs.size() == 2);
  }
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
