// Stand-alone host program over rdycore_amd/csrc/uniform_fields.h (no HIP, no operator): the scan and every transition of the
// uniform-field rules, one "PASS <name>" / "FAIL <name>" line per check.  Built under the address and undefined-behaviour
// sanitizers and run directly by tests/test_uniform_fields_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "uniform_fields.h"

using namespace rdyhip;

static int failures = 0;
static void check(const char *name, bool ok) {
  printf("%s %s\n", ok ? "PASS" : "FAIL", name);
  if (!ok) ++failures;
}
static double from_bits(uint64_t b) {
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

// the scan on arrays of n elements, below and above the size from which it runs in pieces
static void scan_checks(const char *tag, int64_t n) {
  char                name[96];
  std::vector<double> v((size_t)n, 0.015);
  uint64_t            pat = 1;
  snprintf(name, sizeof name, "scan_uniform_%s", tag);
  check(name, uniform_scan(v.data(), n, 1, &pat) && pat == double_bits(0.015));
  v[(size_t)n - 1] = 0.016;
  snprintf(name, sizeof name, "scan_last_differs_%s", tag);
  check(name, !uniform_scan(v.data(), n, 1, &pat));
  v[(size_t)n - 1] = 0.015;
  v[0]             = 0.016;
  snprintf(name, sizeof name, "scan_first_differs_%s", tag);
  check(name, !uniform_scan(v.data(), n, 1, &pat));
  v[0] = 0.015;
  // one element in the middle of every piece in turn
  bool ok = true;
  for (int q = 0; q < 4; ++q) {
    const size_t i = (size_t)(n * (2 * q + 1) / 8);
    v[i]           = -0.015;
    ok             = ok && !uniform_scan(v.data(), n, 1, &pat);
    v[i]           = 0.015;
  }
  snprintf(name, sizeof name, "scan_middle_differs_%s", tag);
  check(name, ok && uniform_scan(v.data(), n, 1, &pat));
  // signed zeros
  std::fill(v.begin(), v.end(), 0.0);
  snprintf(name, sizeof name, "scan_plus_zero_%s", tag);
  check(name, uniform_scan(v.data(), n, 1, &pat) && pat == 0);
  v[(size_t)n / 2] = -0.0;
  snprintf(name, sizeof name, "scan_mixed_zeros_%s", tag);
  check(name, !uniform_scan(v.data(), n, 1, &pat));
  std::fill(v.begin(), v.end(), -0.0);
  snprintf(name, sizeof name, "scan_minus_zero_%s", tag);
  check(name, uniform_scan(v.data(), n, 1, &pat) && pat == 0x8000000000000000ull);
  // NaNs: equal payloads are equal, different payloads are not
  const uint64_t nan_a = 0x7ff8000000000001ull, nan_b = 0x7ff8000000000002ull;
  std::fill(v.begin(), v.end(), from_bits(nan_a));
  snprintf(name, sizeof name, "scan_equal_nans_%s", tag);
  check(name, uniform_scan(v.data(), n, 1, &pat) && pat == nan_a);
  v[(size_t)n / 3] = from_bits(nan_b);
  snprintf(name, sizeof name, "scan_unequal_nans_%s", tag);
  check(name, !uniform_scan(v.data(), n, 1, &pat));
}

int main() {
  scan_checks("small", 1000);
  scan_checks("pieces", UNIFORM_SCAN_PARALLEL_MIN + 12345);

  uint64_t pat = 7;
  double   one = 2.5;
  check("scan_n1", uniform_scan(&one, 1, 1, &pat) && pat == double_bits(2.5));
  pat = 7;
  check("scan_n0", !uniform_scan(&one, 0, 1, &pat) && pat == 7 && !uniform_scan(nullptr, 0, 1, &pat));
  check("all_have_pattern_n0", all_have_pattern(nullptr, 0, 1, 123));
  {  // stride 3: component 0 of [n][3] rows, the other components are not looked at
    std::vector<double> rows(3 * 500);
    for (size_t i = 0; i < 500; ++i) rows[3 * i] = 1e-5, rows[3 * i + 1] = (double)i, rows[3 * i + 2] = -(double)i;
    check("scan_stride3", uniform_scan(rows.data(), 500, 3, &pat) && pat == double_bits(1e-5));
    rows[3 * 499] = 2e-5;
    check("scan_stride3_last_differs", !uniform_scan(rows.data(), 500, 3, &pat));
  }
  {
    std::vector<double> z(100, 0.0), s(100, 0.0);
    bool ok = bed_is_flat(z.data(), s.data(), 100) && bed_is_flat(nullptr, nullptr, 0);
    s[99]   = 1e-300;
    ok      = ok && !bed_is_flat(z.data(), s.data(), 100) && !bed_is_flat(s.data(), z.data(), 100);
    s[99]   = -0.0;
    ok      = ok && !bed_is_flat(z.data(), s.data(), 100);
    check("bed_is_flat", ok);
  }

  // ---- the transitions, in sequence
  const int           N = 64;
  std::vector<double> a(N, 0.015), b(N, 0.02), mixed(N, 0.015);
  mixed[N - 1] = 0.02;
  UniformFields f;
  f.start(true, true);
  check("create_all_uniform_plus_zero", f.mask(true) == (UNIFORM_SOURCE | UNIFORM_MANNINGS | UNIFORM_FLAT_BED) && f.source.pattern == 0 && f.mannings.pattern == 0);
  check("source_bit_needs_water_only", f.mask(false) == (UNIFORM_MANNINGS | UNIFORM_FLAT_BED));
  f.start(true, false);
  check("create_sloped_bed", f.mask(true) == (UNIFORM_SOURCE | UNIFORM_MANNINGS));

  UniformField &m = f.mannings;
  m.write_whole(a.data(), N);
  check("whole_write_starts", m.uniform && m.pattern == double_bits(0.015));
  m.write_whole(b.data(), N);
  check("whole_write_restarts_with_new_value", m.uniform && m.pattern == double_bits(0.02));
  m.write_partial(b.data(), 10);
  check("partial_write_of_the_value_keeps", m.uniform && m.pattern == double_bits(0.02));
  m.fill_partial(0.02);
  check("partial_fill_of_the_value_keeps", m.uniform);
  m.write_partial(a.data(), 1);
  check("partial_write_of_another_value_ends", !m.uniform);
  m.write_partial(b.data(), 10);
  check("partial_write_does_not_start", !m.uniform);
  m.fill_partial(0.02);
  check("partial_fill_does_not_start", !m.uniform);
  m.write_whole(mixed.data(), N);
  check("whole_write_of_unequal_values_stays_off", !m.uniform);
  m.fill_whole(0.03);
  check("whole_fill_starts", m.uniform && m.pattern == double_bits(0.03));
  m.fill_partial(0.031);
  check("partial_fill_of_another_value_ends", !m.uniform);
  m.write_whole(a.data(), N);
  m.write_whole(mixed.data(), N);
  check("whole_write_of_unequal_values_ends", !m.uniform);
  m.write_whole(a.data(), N);
  m.write_unseen();
  check("unseen_write_ends", !m.uniform);
  m.write_partial(mixed.data(), N);
  check("partial_write_after_end_stays_off", !m.uniform);
  m.write_whole(a.data(), N);
  check("whole_write_restarts_after_end", m.uniform && m.pattern == double_bits(0.015));
  {  // -0.0 is a value of its own: +0.0 written into cells of a -0.0 field ends the mode
    std::vector<double> nz(N, -0.0), pz(N, 0.0);
    m.write_whole(nz.data(), N);
    const bool started = m.uniform && m.pattern == 0x8000000000000000ull;
    m.write_partial(nz.data(), 5);
    const bool kept = m.uniform;
    m.write_partial(pz.data(), 5);
    check("minus_zero_is_not_plus_zero", started && kept && !m.uniform);
  }
  m.write_whole(a.data(), N);
  m.escape();
  check("escape_ends", !m.uniform && m.escaped);
  m.write_whole(a.data(), N);
  m.fill_whole(0.015);
  check("escape_is_for_good", !m.uniform);
  check("other_fields_are_untouched", f.source.uniform && f.mask(true) == UNIFORM_SOURCE);

  UniformFields off;
  off.start(false, true);
  off.source.write_whole(a.data(), N);
  off.mannings.fill_whole(0.015);
  check("disabled_stays_off", off.mask(true) == 0 && !off.bed.uniform);

  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
