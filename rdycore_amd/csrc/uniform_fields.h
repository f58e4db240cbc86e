// Uniform input fields: the host-side rules by which the first-order / HR tiled kernels may read element 0 of the water
// source, of Manning's n or of the bed slopes instead of streaming the whole plane (KernelArgs::src_mom bits 1-3,
// swe_kernels.h stream_args).  No HIP, no operator: plain C++, so the scan and every transition can be tested on the host
// (tests/test_uniform_fields_cpu.py).  Included by operator_state.h.
//
// "Uniform" means that every owned element holds the same 64-bit pattern: -0.0 is not +0.0, two NaNs are equal only if
// their payloads are.  The device arrays stay allocated and current whatever the mode is -- entering or leaving a mode moves
// no data -- and element 0, written on the stream by the same setters as ever, is the value the kernels read: the host keeps
// the pattern only to judge later writes, it never reaches the device.
#pragma once
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

namespace rdyhip {

// bits of rdyhip_uniform_fields (include/rdyhip.h: RDYHIP_UNIFORM_*)
enum { UNIFORM_SOURCE = 1, UNIFORM_MANNINGS = 2, UNIFORM_FLAT_BED = 4 };

inline uint64_t double_bits(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}

// every one of the n elements v[0], v[step], ... has the pattern `pat`; stops at the first that differs.  n <= 0: true.
inline bool all_have_pattern(const double *v, int64_t n, int64_t step, uint64_t pat) {
  for (int64_t i = 0; i < n; ++i) {
    uint64_t b;
    memcpy(&b, v + i * step, sizeof(b));
    if (b != pat) return false;
  }
  return true;
}

// The scan of a whole-domain write: true, and the pattern in *pat, if all n elements are equal.  n <= 0: false (there is no
// element 0 to stand for the rest).  Stops at the first differing element -- an array of real rain or roughness costs a few
// loads -- and an array that IS uniform is read once, from UNIFORM_SCAN_PARALLEL_MIN elements on in four pieces side by side
// (80 MB of uniform rain per coupling interval: 2 ms instead of 8), each piece giving up as soon as another has found a difference.
constexpr int64_t UNIFORM_SCAN_PARALLEL_MIN = 1 << 20;
constexpr int64_t UNIFORM_SCAN_BLOCK        = 1 << 14;
inline bool uniform_scan(const double *v, int64_t n, int64_t step, uint64_t *pat) {
  if (n <= 0 || !v) return false;
  const uint64_t p = double_bits(v[0]);
  if (n < UNIFORM_SCAN_PARALLEL_MIN) {
    if (!all_have_pattern(v, n, step, p)) return false;
    *pat = p;
    return true;
  }
  // first and last element before any thread is started: the cheapest way out for arrays that differ at either end
  if (double_bits(v[(n - 1) * step]) != p) return false;
  constexpr int     NT = 4;
  std::atomic<bool> differs(false);
  auto piece = [&](int t) {
    const int64_t lo = n * t / NT, hi = n * (t + 1) / NT;
    for (int64_t b = lo; b < hi && !differs.load(std::memory_order_relaxed); b += UNIFORM_SCAN_BLOCK) {
      const int64_t len = (hi - b < UNIFORM_SCAN_BLOCK) ? hi - b : UNIFORM_SCAN_BLOCK;
      if (!all_have_pattern(v + b * step, len, step, p)) differs.store(true, std::memory_order_relaxed);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < NT; ++t) th.emplace_back(piece, t);
  piece(0);
  for (auto &t : th) t.join();
  if (differs.load()) return false;
  *pat = p;
  return true;
}

// One field's mode.  `enabled` = false (RDYHIP_UNIFORM_FIELDS=0, read at create) keeps it off for good, like `escaped`.
struct UniformField {
  bool     enabled = true;
  bool     uniform = false;
  bool     escaped = false;  // rdyhip_field_ptr handed the array out: it may be written behind our back, for the life of the operator
  uint64_t pattern = 0;

  bool can_hold() const { return enabled && !escaped; }
  // at create: the array has just been zeroed (or, for the static bed, scanned)
  void start(bool on, bool is_uniform, uint64_t pat) {
    enabled = on;
    escaped = false;
    uniform = on && is_uniform;
    pattern = pat;
  }
  // a host write of all owned elements: the mode starts, restarts with a new value, or ends
  void write_whole(const double *v, int64_t n, int64_t step = 1) {
    uint64_t p = 0;
    uniform    = can_hold() && uniform_scan(v, n, step, &p);
    if (uniform) pattern = p;
  }
  // ... of some of them (an id list, or fewer values than owned cells): kept only if every value is the one all cells hold
  void write_partial(const double *v, int64_t n, int64_t step = 1) {
    if (uniform && !all_have_pattern(v, n, step, pattern)) uniform = false;
  }
  // fills with a host scalar: over all owned cells like a whole write of equal values, over some like a partial one
  void fill_whole(double value) {
    uniform = can_hold();
    if (uniform) pattern = double_bits(value);
  }
  void fill_partial(double value) {
    if (uniform && double_bits(value) != pattern) uniform = false;
  }
  // a write whose values the host cannot see (a device array, a device-side gather)
  void write_unseen() { uniform = false; }
  void escape() {
    escaped = true;
    uniform = false;
  }
};

// The three fields of an operator and what a launch and rdyhip_uniform_fields make of them.
struct UniformFields {
  UniformField source, mannings, bed;  // source: component 0 of the external source

  // flat: every dzdx and dzdy of the layout is +0.0 (the bed is static: it has no writer)
  void start(bool on, bool flat) {
    source.start(on, true, 0);  // the arrays are zeroed at create
    mannings.start(on, true, 0);
    bed.start(on, flat, 0);
  }
  // water_only: the operator's water-only mode (the source bit is honoured only there: element 0 of the water plane stands for
  // all cells; element 0 of the [owned][3] array at stride 3 is not read that way)
  int32_t mask(bool water_only) const {
    return (source.uniform && water_only ? UNIFORM_SOURCE : 0) | (mannings.uniform ? UNIFORM_MANNINGS : 0) | (bed.uniform ? UNIFORM_FLAT_BED : 0);
  }
};

// a bed is flat if both slope arrays hold +0.0 and nothing else
inline bool bed_is_flat(const double *dzdx, const double *dzdy, int64_t n) {
  return all_have_pattern(dzdx, n, 1, 0) && all_have_pattern(dzdy, n, 1, 0);
}

}  // namespace rdyhip
