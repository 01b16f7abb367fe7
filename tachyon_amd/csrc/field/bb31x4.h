// BabyBear4 = BabyBear[x] / (x^4 - 11), host and device: the quartic extension
// the FRI challenges live in (non-residue 11, the reference's
// baby_bear/internal/BUILD.bazel).  An element is 4 stored Montgomery words
// c0..c3 (c0 + c1 x + c2 x^2 + c3 x^3), each canonical in [0, p), 16 bytes:
// the layout ExtensionFieldMerkleTreeMMCS flattens to.
#pragma once
#include <cstdint>

#include "bb31.h"

namespace tachyon_amd::bb31x4 {

using bb31::kP;

inline constexpr uint32_t kW = 11;  // the non-residue

struct alignas(16) Fp4 {
  uint32_t c[4];
};

// Montgomery reduction of a lazily accumulated sum t < 2^32 p: with
// m = t (-p^-1) mod 2^32, t + m p < 2^32 p + 2^32 p = 2^33 p < 2^64 does not
// wrap, and (t + m p) / 2^32 < 2p: one conditional subtraction.  A sum of two
// products of canonical words is below 2 p^2 < 2^32 p (2p < 2^32) and fits; a
// sum of three or four does not (3 p^2 + 2^32 p > 2^64).
BB31_HD uint32_t redc(uint64_t t) {
  const uint32_t m = (uint32_t)t * bb31::kNInv;
  const uint32_t u = (uint32_t)((t + (uint64_t)m * kP) >> 32);
  return u >= kP ? u - kP : u;
}

// a b + c d (Montgomery), the sum below 2 p^2: see redc
BB31_HD uint32_t dot2(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return redc((uint64_t)a * b + (uint64_t)c * d);
}

// 11 a for canonical a (Montgomery form is kept: 11 (x R) = (11 x) R):
// t = 11 a < 11 p < 2^35, reduced by the quotient estimate q = t >> 31.
// q <= t / p (p < 2^31) and q > t / 2^31 - 1, so the remainder
// t - q p < t (1 - p / 2^31) + p < 11 p 2^-4 + p < 2p: one conditional
// subtraction.
BB31_HD uint32_t mul_w(uint32_t a) {
  const uint64_t t = (uint64_t)a * kW;
  const uint32_t r = (uint32_t)(t - (t >> 31) * kP);
  return r >= kP ? r - kP : r;
}

BB31_HD Fp4 zero() { return Fp4{{0, 0, 0, 0}}; }
BB31_HD Fp4 one() { return Fp4{{bb31::kR, 0, 0, 0}}; }
BB31_HD Fp4 from_base(uint32_t a) { return Fp4{{a, 0, 0, 0}}; }
BB31_HD bool is_zero(const Fp4& a) { return (a.c[0] | a.c[1] | a.c[2] | a.c[3]) == 0; }
BB31_HD bool equal(const Fp4& a, const Fp4& b) {
  return a.c[0] == b.c[0] && a.c[1] == b.c[1] && a.c[2] == b.c[2] && a.c[3] == b.c[3];
}

BB31_HD Fp4 add(const Fp4& a, const Fp4& b) {
  return Fp4{{bb31::add(a.c[0], b.c[0]), bb31::add(a.c[1], b.c[1]), bb31::add(a.c[2], b.c[2]),
              bb31::add(a.c[3], b.c[3])}};
}

BB31_HD Fp4 sub(const Fp4& a, const Fp4& b) {
  return Fp4{{bb31::sub(a.c[0], b.c[0]), bb31::sub(a.c[1], b.c[1]), bb31::sub(a.c[2], b.c[2]),
              bb31::sub(a.c[3], b.c[3])}};
}

BB31_HD Fp4 neg(const Fp4& a) {
  return Fp4{{bb31::sub(0, a.c[0]), bb31::sub(0, a.c[1]), bb31::sub(0, a.c[2]), bb31::sub(0, a.c[3])}};
}

// extension x base: four base products
BB31_HD Fp4 mul_base(const Fp4& a, uint32_t b) {
  return Fp4{{bb31::mul(a.c[0], b), bb31::mul(a.c[1], b), bb31::mul(a.c[2], b), bb31::mul(a.c[3], b)}};
}

// Schoolbook product with x^4 = 11.  The coefficient
//   a0 b0 + 11 (a1 b3 + a2 b2 + a3 b1)
// is a sum of four products and does not fit one reduction, so it is split:
// 11 b1, 11 b2, 11 b3 are formed first (canonical, mul_w), and every
// coefficient is then two sums of two products, each below 2 p^2 (dot2), added
// canonically.  16 products and 8 reductions.
BB31_HD Fp4 mul(const Fp4& a, const Fp4& b) {
  const uint32_t w1 = mul_w(b.c[1]), w2 = mul_w(b.c[2]), w3 = mul_w(b.c[3]);
  Fp4 r;
  r.c[0] = bb31::add(dot2(a.c[0], b.c[0], a.c[1], w3), dot2(a.c[2], w2, a.c[3], w1));
  r.c[1] = bb31::add(dot2(a.c[0], b.c[1], a.c[1], b.c[0]), dot2(a.c[2], w3, a.c[3], w2));
  r.c[2] = bb31::add(dot2(a.c[0], b.c[2], a.c[1], b.c[1]), dot2(a.c[2], b.c[0], a.c[3], w3));
  r.c[3] = bb31::add(dot2(a.c[0], b.c[3], a.c[1], b.c[2]), dot2(a.c[2], b.c[1], a.c[3], b.c[0]));
  return r;
}

// a^2: the symmetric terms once, doubled canonically.  With w_i = 11 a_i:
//   c0 = a0^2 + a2 w2 + 2 a1 w3     c1 = 2 (a0 a1 + a2 w3)
//   c2 = a1^2 + a3 w3 + 2 a0 a2     c3 = 2 (a0 a3 + a1 a2)
// every dot2 a sum of two products, below 2 p^2.
BB31_HD Fp4 square(const Fp4& a) {
  const uint32_t w2 = mul_w(a.c[2]), w3 = mul_w(a.c[3]);
  const uint32_t t0 = bb31::mul(a.c[1], w3), t2 = bb31::mul(a.c[0], a.c[2]);
  const uint32_t t1 = dot2(a.c[0], a.c[1], a.c[2], w3), t3 = dot2(a.c[0], a.c[3], a.c[1], a.c[2]);
  Fp4 r;
  r.c[0] = bb31::add(dot2(a.c[0], a.c[0], a.c[2], w2), bb31::add(t0, t0));
  r.c[1] = bb31::add(t1, t1);
  r.c[2] = bb31::add(dot2(a.c[1], a.c[1], a.c[3], w3), bb31::add(t2, t2));
  r.c[3] = bb31::add(t3, t3);
  return r;
}

// base^e
BB31_HD Fp4 pow(Fp4 base, uint64_t e) {
  Fp4 r = one();
  while (e) {
    if (e & 1) r = mul(r, base);
    base = square(base);
    e >>= 1;
  }
  return r;
}

// a^-1 through the tower K = F[y] / (y^2 - 11), y = x^2: a = A + B x with
// A = a0 + a2 y, B = a1 + a3 y, norm N = A^2 - y B^2 = n0 + n1 y in K,
// N^-1 = (n0 - n1 y) / (n0^2 - 11 n1^2) with one base inversion, and
// a^-1 = (A - B x) N^-1.  The inverse of 0 is 0 (the base inversion is a power,
// and 0^(p-2) = 0): callers that must refuse a zero test for it themselves.
BB31_HD Fp4 inverse(const Fp4& a) {
  using bb31::add;
  using bb31::sub;
  const uint32_t w2 = mul_w(a.c[2]), w3 = mul_w(a.c[3]);
  const uint32_t a1w3 = bb31::mul(a.c[1], w3), a0a2 = bb31::mul(a.c[0], a.c[2]);
  // n0 = a0^2 + 11 a2^2 - 2 * 11 a1 a3,  n1 = 2 a0 a2 - a1^2 - 11 a3^2
  const uint32_t n0 = sub(dot2(a.c[0], a.c[0], a.c[2], w2), add(a1w3, a1w3));
  const uint32_t n1 = sub(add(a0a2, a0a2), dot2(a.c[1], a.c[1], a.c[3], w3));
  const uint32_t d = sub(bb31::mul(n0, n0), mul_w(bb31::mul(n1, n1)));
  const uint32_t di = bb31::inverse(d);
  const uint32_t i0 = bb31::mul(n0, di), i1 = sub(0, bb31::mul(n1, di));
  const uint32_t wi1 = mul_w(i1);
  Fp4 r;
  r.c[0] = dot2(a.c[0], i0, a.c[2], wi1);                // A N^-1 = (a0 i0 + 11 a2 i1) + (a0 i1 + a2 i0) y
  r.c[2] = dot2(a.c[0], i1, a.c[2], i0);
  r.c[1] = sub(0, dot2(a.c[1], i0, a.c[3], wi1));        // -B N^-1
  r.c[3] = sub(0, dot2(a.c[1], i1, a.c[3], i0));
  return r;
}

}  // namespace tachyon_amd::bb31x4
