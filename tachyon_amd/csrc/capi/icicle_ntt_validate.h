// Argument checks of the tachyon_mi355x_icicle_ntt_* entry points
// (include/tachyon_mi355x.h): host-only C++ with no HIP dependency, so the
// refusal rules can be compiled and run on their own.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../../include/tachyon_mi355x.h"

namespace tachyon_amd::icicle_ntt {

// IcicleNTTOptions' defaults (icicle_ntt.h:43-51)
inline tachyon_mi355x_icicle_ntt_options default_options() {
  tachyon_mi355x_icicle_ntt_options o;
  o.fast_twiddles_mode = 1;
  o.batch_size = 1;
  o.columns_batch = 0;
  o.ordering = 0;
  o.are_inputs_on_device = 0;
  o.are_outputs_on_device = 0;
  o.is_async = 0;
  return o;
}

// batch >= 1, no column batches, natural order in and out, one in-place pointer
inline bool options_ok(const tachyon_mi355x_icicle_ntt_options& o) {
  return o.batch_size >= 1 && o.columns_batch == 0 && o.ordering == 0 &&
         (o.are_inputs_on_device != 0) == (o.are_outputs_on_device != 0);
}

// baby_bear (field 4): as above, and columns_batch 0 or 1
inline bool options_ok_columns(const tachyon_mi355x_icicle_ntt_options& o) {
  return o.batch_size >= 1 && (o.columns_batch == 0 || o.columns_batch == 1) && o.ordering == 0 &&
         (o.are_inputs_on_device != 0) == (o.are_outputs_on_device != 0);
}

// baby_bear's BigInt<1>: 8 little-endian bytes holding a canonical value in
// [1, modulus); false for 0, for values >= modulus and for any bit above 32
inline bool small_coset(const void* bytes, uint32_t modulus, uint32_t* out) {
  const unsigned char* b = static_cast<const unsigned char*>(bytes);
  uint64_t v = 0;
  for (int i = 7; i >= 0; --i) v = (v << 8) | b[i];
  if (v == 0 || v >= modulus) return false;
  *out = (uint32_t)v;
  return true;
}

// log2(size) for a power of two in [1, 2^log_order], -1 for anything else
inline int size_log(size_t size, int log_order) {
  if (log_order < 0 || size == 0 || (size & (size - 1)) != 0) return -1;
  int l = 0;
  while ((size_t(1) << l) < size) ++l;
  return l <= log_order ? l : -1;
}

// 32 little-endian bytes -> 8 words
inline void load_words(const void* bytes, uint32_t out[8]) {
  const unsigned char* b = static_cast<const unsigned char*>(bytes);
  for (int i = 0; i < 8; ++i)
    out[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
             ((uint32_t)b[4 * i + 3] << 24);
}

// v < p, both 8 little-endian words
inline bool below(const uint32_t v[8], const uint32_t p[8]) {
  for (int i = 7; i >= 0; --i)
    if (v[i] != p[i]) return v[i] < p[i];
  return false;
}

inline bool is_zero(const uint32_t v[8]) {
  uint32_t acc = 0;
  for (int i = 0; i < 8; ++i) acc |= v[i];
  return acc == 0;
}

// a coset offset in canonical form: 0 < v < modulus
inline bool coset_ok(const uint32_t v[8], const uint32_t modulus[8]) { return !is_zero(v) && below(v, modulus); }

}  // namespace tachyon_amd::icicle_ntt
