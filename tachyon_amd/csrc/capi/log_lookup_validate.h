// Argument checks of tachyon_mi355x_log_lookup_m_polys and
// tachyon_mi355x_log_lookup_grand_sums (include/tachyon_mi355x.h): host-only
// C++ with no HIP dependency, so the refusal rules can be compiled and run on
// their own.  Nothing here touches the GPU or dereferences a column: only the
// descriptor arrays are read and the columns' address ranges compared.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../../include/tachyon_mi355x.h"

namespace tachyon_amd::ll_validate {

inline constexpr size_t kElemBytes = 32;
inline constexpr size_t kMaxRows = (size_t)1 << 30;

inline bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// field, n (a power of two in [2, 2^30]) and 0 < usable_rows < n
inline bool shape_ok(int field, size_t n, size_t usable_rows) {
  if (field != 0 && field != 2) return false;
  if (n < 2 || n > kMaxRows || (n & (n - 1)) != 0) return false;
  return usable_rows != 0 && usable_rows < n;
}

// every lookup has at least one input, and no column pointer is null
inline bool lookups_ok(const tachyon_mi355x_log_lookup* lookups, size_t count) {
  if (count != 0 && !lookups) return false;
  for (size_t l = 0; l < count; ++l) {
    if (lookups[l].num_inputs == 0 || !lookups[l].inputs || !lookups[l].table) return false;
    for (size_t k = 0; k < lookups[l].num_inputs; ++k)
      if (!lookups[l].inputs[k]) return false;
  }
  return true;
}

// no output is null, overlaps another output, an input, a table or an `extra` column (the m of the grand sums)
inline bool outputs_ok(size_t n, const tachyon_mi355x_log_lookup* lookups, const void* const* extra, size_t count,
                       void* const* out) {
  if (count != 0 && !out) return false;
  const size_t bytes = n * kElemBytes;
  for (size_t i = 0; i < count; ++i) {
    if (!out[i]) return false;
    for (size_t j = 0; j < i; ++j)
      if (overlap(out[i], out[j], bytes)) return false;
    for (size_t l = 0; l < count; ++l) {
      for (size_t k = 0; k < lookups[l].num_inputs; ++k)
        if (overlap(out[i], lookups[l].inputs[k], bytes)) return false;
      if (overlap(out[i], lookups[l].table, bytes)) return false;
      if (extra && overlap(out[i], extra[l], bytes)) return false;
    }
  }
  return true;
}

// True when tachyon_mi355x_log_lookup_m_polys can run
inline bool check_m_polys(int field, size_t n, size_t usable_rows, const tachyon_mi355x_log_lookup* lookups,
                          size_t count, void* const* out_m) {
  return shape_ok(field, n, usable_rows) && lookups_ok(lookups, count) &&
         outputs_ok(n, lookups, nullptr, count, out_m);
}

// The blinding values one call takes: n - usable_rows - 1 per phi
inline size_t blind_elems(size_t n, size_t usable_rows, size_t count) { return count * (n - usable_rows - 1); }

// True when tachyon_mi355x_log_lookup_grand_sums can run.  The C entry point
// takes blinds as a pointer alone and passes blind_elems() itself for
// num_blinds; a caller that knows the length of its array (the Python
// binding, a C++ wrapper) passes that, and a wrong length is refused here.
inline bool check_grand_sums(int field, size_t n, size_t usable_rows, const void* beta,
                             const tachyon_mi355x_log_lookup* lookups, const void* const* m, size_t count,
                             const void* blinds, size_t num_blinds, void* const* out_phi) {
  if (!shape_ok(field, n, usable_rows) || !beta || !lookups_ok(lookups, count)) return false;
  if (num_blinds != blind_elems(n, usable_rows, count)) return false;
  if (num_blinds != 0 && !blinds) return false;
  if (count != 0 && !m) return false;
  for (size_t l = 0; l < count; ++l)
    if (!m[l]) return false;
  return outputs_ok(n, lookups, m, count, out_phi);
}

}  // namespace tachyon_amd::ll_validate
