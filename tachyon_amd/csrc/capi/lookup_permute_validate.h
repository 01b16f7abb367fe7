// Argument checks of tachyon_mi355x_lookup_permute_pairs (include/
// tachyon_mi355x.h): host-only C++ with no HIP dependency, so the refusal
// rules can be compiled and run on their own.  Nothing here touches the GPU or
// dereferences a column: only the descriptor and pointer arrays are read and
// the columns' address ranges compared.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../../include/tachyon_mi355x.h"

namespace tachyon_amd::lp_validate {

inline constexpr size_t kElemBytes = 32;
inline constexpr size_t kMaxRows = (size_t)1 << 30;

// two ranges of `bytes` bytes; by the distance of their starts, so that no sum can wrap
inline bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return (x < y ? y - x : x - y) < bytes;
}

// field, n (a power of two in [2, 2^30]) and 0 < usable_rows < n
inline bool shape_ok(int field, size_t n, size_t usable_rows) {
  if (field != 0 && field != 2) return false;
  if (n < 2 || n > kMaxRows || (n & (n - 1)) != 0) return false;
  return usable_rows != 0 && usable_rows < n;
}

// no column pointer is null
inline bool pairs_ok(const tachyon_mi355x_lookup_pair* pairs, size_t count) {
  if (count != 0 && !pairs) return false;
  for (size_t l = 0; l < count; ++l)
    if (!pairs[l].input || !pairs[l].table) return false;
  return true;
}

// no output is null, overlaps another output (of either list) or a column of the call
inline bool outputs_ok(size_t n, const tachyon_mi355x_lookup_pair* pairs, size_t count, void* const* out_input,
                       void* const* out_table) {
  if (count != 0 && (!out_input || !out_table)) return false;
  const size_t bytes = n * kElemBytes;
  for (size_t i = 0; i < 2 * count; ++i) {
    const void* out = i < count ? out_input[i] : out_table[i - count];
    if (!out) return false;
    for (size_t j = 0; j < i; ++j)
      if (overlap(out, j < count ? out_input[j] : out_table[j - count], bytes)) return false;
    for (size_t l = 0; l < count; ++l)
      if (overlap(out, pairs[l].input, bytes) || overlap(out, pairs[l].table, bytes)) return false;
  }
  return true;
}

// The blinding values one call takes: per pair n - usable_rows for A', then as many for S'
inline size_t blind_elems(size_t n, size_t usable_rows, size_t count) { return count * 2 * (n - usable_rows); }

// True when tachyon_mi355x_lookup_permute_pairs can run.  The C entry point
// takes blinds as a pointer alone and passes blind_elems() itself for
// num_blinds; a caller that knows the length of its array (the Python
// binding, a C++ wrapper) passes that, and a wrong length is refused here.
inline bool check_permute_pairs(int field, size_t n, size_t usable_rows, const tachyon_mi355x_lookup_pair* pairs,
                                size_t count, const void* blinds, size_t num_blinds, void* const* out_input,
                                void* const* out_table) {
  if (!shape_ok(field, n, usable_rows) || !pairs_ok(pairs, count)) return false;
  if (num_blinds != blind_elems(n, usable_rows, count)) return false;
  if (num_blinds != 0 && !blinds) return false;
  return outputs_ok(n, pairs, count, out_input, out_table);
}

}  // namespace tachyon_amd::lp_validate
