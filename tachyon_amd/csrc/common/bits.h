// Bit helpers of the host-side argument checks (capi/*_validate.h): host-only
// C++ with no HIP dependency.
#pragma once
#include <cstddef>

namespace tachyon_amd::bits {

inline bool is_pow2(size_t n) { return n != 0 && (n & (n - 1)) == 0; }

// the least power of two >= n
inline size_t bit_ceil(size_t n) {
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// ceil(log2(n)) for n >= 1: log2 of a power of two
inline unsigned ceil_log2(size_t n) {
  unsigned l = 0;
  while ((size_t(1) << l) < n) ++l;
  return l;
}

// x reversed over `bits` bits
inline size_t bit_reverse(size_t x, unsigned bits) {
  size_t r = 0;
  for (unsigned b = 0; b < bits; ++b) r |= ((x >> b) & 1) << (bits - 1 - b);
  return r;
}

}  // namespace tachyon_amd::bits
