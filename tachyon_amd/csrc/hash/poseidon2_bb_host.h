// Poseidon2 over BabyBear, width 16, on the host: the permutation of
// poseidon2_bb.h word for word (the same field code, the same constants, the
// same order of additions), as plain C++ with no HIP dependency.  It serves the
// transcript (fri/challenger_bb.h), where one state at a time is permuted
// between two device steps; batches belong on the device.
#pragma once
#include <cstdint>

#include "../field/bb31.h"
#include "poseidon2_bb_constants.h"

namespace tachyon_amd::poseidon2_bb_host {

namespace c = poseidon2_bb;

inline constexpr int kHorizen = 0, kPlonky3 = 1;  // poseidon2_bb::External

inline constexpr uint32_t kRoundConstants[c::kNumConstants] = {POSEIDON2_BB_ROUND_CONSTANTS};
inline constexpr int kShift[15] = {POSEIDON2_BB_INTERNAL_SHIFTS};

inline uint32_t dbl(uint32_t a) { return bb31::add(a, a); }

inline uint32_t sbox(uint32_t x) {
  const uint32_t x2 = bb31::mul(x, x);
  const uint32_t x3 = bb31::mul(x2, x);
  const uint32_t x4 = bb31::mul(x2, x2);
  return bb31::mul(x3, x4);
}

inline void m4(int external, uint32_t* x) {
  using bb31::add;
  if (external == kHorizen) {
    const uint32_t t0 = add(x[0], x[1]);
    const uint32_t t1 = add(x[2], x[3]);
    const uint32_t t2 = add(dbl(x[1]), t1);
    const uint32_t t3 = add(dbl(x[3]), t0);
    const uint32_t t4 = add(dbl(dbl(t1)), t3);
    const uint32_t t5 = add(dbl(dbl(t0)), t2);
    x[0] = add(t3, t5);
    x[1] = t5;
    x[2] = add(t2, t4);
    x[3] = t4;
  } else {
    const uint32_t t01 = add(x[0], x[1]);
    const uint32_t t23 = add(x[2], x[3]);
    const uint32_t t0123 = add(t01, t23);
    const uint32_t t01123 = add(t0123, x[1]);
    const uint32_t t01233 = add(t0123, x[3]);
    const uint32_t y3 = add(t01233, dbl(x[0]));
    const uint32_t y1 = add(t01123, dbl(x[2]));
    x[0] = add(t01123, t01);
    x[1] = y1;
    x[2] = add(t01233, t23);
    x[3] = y3;
  }
}

inline void external_layer(int external, uint32_t* s) {
  for (int b = 0; b < 4; ++b) m4(external, s + 4 * b);
  for (int r = 0; r < 4; ++r) {
    const uint32_t sum = bb31::add(bb31::add(s[r], s[r + 4]), bb31::add(s[r + 8], s[r + 12]));
    for (int b = 0; b < 4; ++b) s[4 * b + r] = bb31::add(s[4 * b + r], sum);
  }
}

// t 2^-32 mod p for t < 2^47 (poseidon2_bb.h's reduce64)
inline uint32_t reduce64(uint64_t t) {
  const uint32_t m = (uint32_t)t * bb31::kNInv;
  const uint32_t u = (uint32_t)((t + (uint64_t)m * bb31::kP) >> 32);
  return u >= bb31::kP ? u - bb31::kP : u;
}

inline void internal_layer(uint32_t* s) {
  uint64_t sum = 0;
  for (int i = 0; i < 16; ++i) sum += s[i];
  s[0] = reduce64(sum + 2 * (uint64_t)(bb31::kP - s[0]));
  for (int i = 1; i < 16; ++i) s[i] = reduce64(sum + ((uint64_t)s[i] << kShift[i - 1]));
}

inline void full_rounds(int external, uint32_t* s, int begin) {
  for (int r = 0; r < c::kHalfFullRounds; ++r) {
    const uint32_t* k = kRoundConstants + begin + 16 * r;
    for (int i = 0; i < 16; ++i) s[i] = sbox(bb31::add(s[i], k[i]));
    external_layer(external, s);
  }
}

// 16 canonical Montgomery words in place; external: kHorizen or kPlonky3
inline void permute(int external, uint32_t* s) {
  external_layer(external, s);
  full_rounds(external, s, 0);
  for (int r = 0; r < c::kPartialRounds; ++r) {
    s[0] = sbox(bb31::add(s[0], kRoundConstants[c::kBeginPartial + r]));
    internal_layer(s);
  }
  full_rounds(external, s, c::kBeginLastFull);
}

}  // namespace tachyon_amd::poseidon2_bb_host
