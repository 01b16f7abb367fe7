// Poseidon2 over BabyBear, width 16, x^7, 4 + 13 + 4 rounds
// (poseidon2.h:46-67, Poseidon2Params<BabyBear, 15, 7>): the permutation as an
// inline function on 16 words, on the stored Montgomery words of field/bb31.h.
// One body for host and device (BB31_HD): on the device one state per lane in
// 16 registers; on the host one state at a time for the transcript
// (fri/challenger_bb.h), with any host compiler and no HIP.
//
// The rounds are loops over a table of constants.  On the device the table is
// __constant__ and the round index uniform, so the constants arrive by scalar
// loads, and the kernel holds one full-round body and one partial-round body
// instead of 21 unrolled rounds (which would not fit the instruction cache).
// The host reads a constexpr table built from the same macro.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define POSEIDON2_BB_UNROLL _Pragma("unroll")
#define POSEIDON2_BB_NO_UNROLL _Pragma("unroll 1")
#else
#define POSEIDON2_BB_UNROLL
#define POSEIDON2_BB_NO_UNROLL
#endif

#include <cstdint>

#include "../field/bb31.h"
#include "poseidon2_bb_constants.h"

namespace tachyon_amd::poseidon2_bb {

enum External : int { kHorizen = 0, kPlonky3 = 1 };

// The table the pass being compiled reads.  The device's accessor is
// __device__ alone: a __constant__ named in a host-and-device function counts
// as used by the host, which costs every access an indirection.
#if defined(__HIP_DEVICE_COMPILE__)
static __constant__ uint32_t kRoundConstants[kNumConstants] = {POSEIDON2_BB_ROUND_CONSTANTS};
__device__ __forceinline__ const uint32_t* round_constants() { return kRoundConstants; }
#else
inline constexpr uint32_t kHostRoundConstants[kNumConstants] = {POSEIDON2_BB_ROUND_CONSTANTS};
inline const uint32_t* round_constants() { return kHostRoundConstants; }
#endif

BB31_HD uint32_t dbl(uint32_t a) { return bb31::add(a, a); }

// x^7 in 4 products
BB31_HD uint32_t sbox(uint32_t x) {
  const uint32_t x2 = bb31::mul(x, x);
  const uint32_t x3 = bb31::mul(x2, x);
  const uint32_t x4 = bb31::mul(x2, x2);
  return bb31::mul(x3, x4);
}

// The 4 x 4 block on lanes x[0..4), additions only.
//   Horizen: rows (5 7 1 3), (4 6 1 1), (1 3 5 7), (1 1 4 6)
//   Plonky3: the circulant (2 3 1 1)
template <int EXT>
BB31_HD void m4(uint32_t* x) {
  using bb31::add;
  if constexpr (EXT == kHorizen) {
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

// poseidon2_external_matrix.h:21-63: M4 on each block, then lane i gains the
// sum of the lanes congruent to i mod 4.
template <int EXT>
BB31_HD void external_layer(uint32_t* s) {
  POSEIDON2_BB_UNROLL
  for (int b = 0; b < 4; ++b) m4<EXT>(s + 4 * b);
  POSEIDON2_BB_UNROLL
  for (int r = 0; r < 4; ++r) {
    const uint32_t sum = bb31::add(bb31::add(s[r], s[r + 4]), bb31::add(s[r + 8], s[r + 12]));
    POSEIDON2_BB_UNROLL
    for (int b = 0; b < 4; ++b) s[4 * b + r] = bb31::add(s[4 * b + r], sum);
  }
}

// t 2^-32 mod p for t < 2^47: t + m p < 2^47 + 2^32 p is a multiple of 2^32
// and the quotient is below p + 2^15 < 2p.
BB31_HD uint32_t reduce64(uint64_t t) {
  const uint32_t m = (uint32_t)t * bb31::kNInv;
  const uint32_t u = (uint32_t)((t + (uint64_t)m * bb31::kP) >> 32);
  return u >= bb31::kP ? u - bb31::kP : u;
}

// poseidon2_plonky3_internal_matrix.h:41-66: with S the integer sum of the 16
// stored words (< 2^35), lane 0 becomes (S - 2 v0) 2^-32 and lane i >= 1
// (S + (v_i << shift)) 2^-32 (< 2^47 before the reduction); no products.
BB31_HD void internal_layer(uint32_t* s) {
  constexpr int kShift[15] = {POSEIDON2_BB_INTERNAL_SHIFTS};
  uint64_t sum = 0;
  POSEIDON2_BB_UNROLL
  for (int i = 0; i < 16; ++i) sum += s[i];
  s[0] = reduce64(sum + 2 * (uint64_t)(bb31::kP - s[0]));
  POSEIDON2_BB_UNROLL
  for (int i = 1; i < 16; ++i) s[i] = reduce64(sum + ((uint64_t)s[i] << kShift[i - 1]));
}

template <int EXT>
BB31_HD void full_rounds(uint32_t* s, int begin) {
  POSEIDON2_BB_NO_UNROLL
  for (int r = 0; r < kHalfFullRounds; ++r) {
    const uint32_t* c = round_constants() + begin + 16 * r;
    POSEIDON2_BB_UNROLL
    for (int i = 0; i < 16; ++i) s[i] = sbox(bb31::add(s[i], c[i]));
    external_layer<EXT>(s);
  }
}

// 16 canonical Montgomery words in place
template <int EXT>
BB31_HD void permute(uint32_t* s) {
  external_layer<EXT>(s);
  full_rounds<EXT>(s, 0);
  POSEIDON2_BB_NO_UNROLL
  for (int r = 0; r < kPartialRounds; ++r) {
    s[0] = sbox(bb31::add(s[0], round_constants()[kBeginPartial + r]));
    internal_layer(s);
  }
  full_rounds<EXT>(s, kBeginLastFull);
}

// the same for an `external` known only at run time (the transcript's)
BB31_HD void permute(int external, uint32_t* s) { external == kHorizen ? permute<kHorizen>(s) : permute<kPlonky3>(s); }

}  // namespace tachyon_amd::poseidon2_bb
