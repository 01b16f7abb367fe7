// Device helpers for the 8-limb scalar fields: 16-byte element access, the
// order of canonical keys, wave shuffles and the workgroup's product and sum
// scans.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tachyon_amd {

// An element is two 16-byte halves (V: a vector of four 32-bit words)
template <class Fr, class V>
__device__ __forceinline__ Fr unpack_fr(const V& lo, const V& hi) {
  static_assert(sizeof(Fr) == 32 && sizeof(V) == 16, "8-limb scalar fields");
  Fr r;
  r.v[0] = lo.x, r.v[1] = lo.y, r.v[2] = lo.z, r.v[3] = lo.w;
  r.v[4] = hi.x, r.v[5] = hi.y, r.v[6] = hi.z, r.v[7] = hi.w;
  return r;
}

template <class Fr>
__device__ __forceinline__ void pack_fr(const Fr& x, uint4* lo, uint4* hi) {
  *lo = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  *hi = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// 32-byte elements move as two 16-byte accesses (Fr alone is 4-byte aligned,
// which would make them eight dword accesses)
template <class Fr>
__device__ __forceinline__ Fr load_fr(const Fr* p) {
  const uint4 lo = reinterpret_cast<const uint4*>(p)[0];
  const uint4 hi = reinterpret_cast<const uint4*>(p)[1];
  return unpack_fr<Fr>(lo, hi);
}

// (the two stores are written out, not through pack_fr's pointers: that form
// changed gp_apply_kernel's register allocation, profiles/fr_helpers)
template <class Fr>
__device__ __forceinline__ void store_fr(Fr* p, const Fr& x) {
  reinterpret_cast<uint4*>(p)[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// The order of the canonical integers *key and x: -1, 0, 1 for key <, =, > x;
// most significant limb first, the low half read only behind an equal high one
template <class Fr>
__device__ __forceinline__ int compare_key(const Fr* key, const Fr& x) {
  const uint4 hi = reinterpret_cast<const uint4*>(key)[1];
  const uint32_t h[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int i = 3; i >= 0; --i)
    if (h[i] != x.v[4 + i]) return h[i] < x.v[4 + i] ? -1 : 1;
  const uint4 lo = reinterpret_cast<const uint4*>(key)[0];
  const uint32_t l[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
  for (int i = 3; i >= 0; --i)
    if (l[i] != x.v[i]) return l[i] < x.v[i] ? -1 : 1;
  return 0;
}

// x of lane src (mod 64)
template <class Fr>
__device__ __forceinline__ Fr shfl_fr(const Fr& x, unsigned src) {
  Fr r;
#pragma unroll
  for (int i = 0; i < Fr::N; ++i) r.v[i] = (uint32_t)__shfl((int)x.v[i], (int)(src & 63), 64);
  return r;
}

// x of lane + d; the lane's own past the wave's end
template <class Fr>
__device__ __forceinline__ Fr shfl_down_fr(const Fr& x, unsigned d) {
  Fr r;
#pragma unroll
  for (int i = 0; i < Fr::N; ++i) r.v[i] = (uint32_t)__shfl_down((int)x.v[i], d, 64);
  return r;
}

// Exclusive product scan over a workgroup of kBlock threads in thread order
// (kReverse: from the last thread down): returns the product of x over the
// threads before this one, *total the product over all of them (the same in
// every thread).  lds: kBlock / 64 elements; the leading barrier lets the
// previous use drain.
template <class Fr, unsigned kBlock, bool kReverse>
__device__ __forceinline__ Fr block_scan_mul(const Fr& x, Fr* lds, Fr* total) {
  constexpr unsigned kWaves = kBlock / 64;
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned pos = kReverse ? 63 - lane : lane;
  // Kogge-Stone over the wave: s = product over the positions <= pos
  Fr s = x;
  for (unsigned d = 1; d < 64; d <<= 1) {
    const Fr t = shfl_fr(s, kReverse ? lane + d : lane - d);
    const Fr m = s * t;
    if (pos >= d) s = m;
  }
  Fr e = shfl_fr(s, kReverse ? lane + 1 : lane - 1);
  if (pos == 0) e = Fr::one();
  __syncthreads();
  if (pos == 63) lds[wave] = s;
  __syncthreads();
  Fr before = Fr::one(), acc = Fr::one();
  for (unsigned i = 0; i < kWaves; ++i) {
    const unsigned w = kReverse ? kWaves - 1 - i : i;
    if (w == wave) before = acc;
    acc = acc * lds[w];
  }
  *total = acc;
  return before * e;
}

// The same scan with sums, in thread order: returns the sum of x over the
// threads before this one, *total the sum over all of them.
template <class Fr, unsigned kBlock>
__device__ __forceinline__ Fr block_scan_add(const Fr& x, Fr* lds, Fr* total) {
  constexpr unsigned kWaves = kBlock / 64;
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Fr s = x;
  for (unsigned d = 1; d < 64; d <<= 1) {
    const Fr m = s + shfl_fr(s, lane - d);
    if (lane >= d) s = m;
  }
  Fr e = shfl_fr(s, lane - 1);
  if (lane == 0) e = Fr::zero();
  __syncthreads();
  if (lane == 63) lds[wave] = s;
  __syncthreads();
  Fr before = Fr::zero(), acc = Fr::zero();
  for (unsigned i = 0; i < kWaves; ++i) {
    if (i == wave) before = acc;
    acc = acc + lds[i];
  }
  *total = acc;
  return before + e;
}

}  // namespace tachyon_amd
