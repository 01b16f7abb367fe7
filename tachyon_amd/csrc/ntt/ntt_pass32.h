// The NTT pass over 8 x 32-bit limbs (any field): the tile constants, the
// pass modes, the twiddle forms, PassArgs and dif_pass_kernel.  Device code
// of ntt.hip's translation unit: included there only, first of its three
// kernel headers (ntt_pass32.h, ntt_pass29.h, ntt_tables.h).
#pragma once
#include "ntt.h"

namespace tachyon_amd::ntt {

namespace {

constexpr unsigned kBlock = 256;
constexpr uint32_t kMaxPassStages = 8;
// Elements per workgroup: 1024 (32 KiB of LDS) = 256 threads x 2^2, so every
// thread owns one radix-4 group per register step and 5 workgroups fit a CU
// (5 waves per SIMD at 88 VGPRs).  2^24 sweep (tools/tune_ntt.py,
// TACHYON_NTT_LDS_ELEMS x TACHYON_NTT_RADIX_LOG): 2048/r3 2.43, 2048/r2 2.44,
// 1024/r2 1.95, 1024/r3 2.82 (half the threads idle), 512/r2 2.54 ms.
constexpr uint32_t kMaxLdsElems = 1024;

enum : uint32_t {
  kLoadCoset = 1,
  kStoreScale = 2,
  kStoreCoset = 4,
  kLoadTw4 = 8,
  kStoreTw4 = 16,
  kLoadXch = 32,
  kStoreXch = 64
};

// Twiddle tables.  BN254 Fr butterflies multiply by a Shoup product
// (Fp::mul_shoup, mont_asm.h shoup_mul_8): an entry is the plain twiddle and
// its quotient floor(w 2^256 / p), 64 bytes -- 13 fewer v_mad_u64_u32, 29
// fewer carry adds and no Montgomery digits per butterfly than a Montgomery
// product by a 32-byte Montgomery twiddle.  BLS12-381 Fr (3p > 2^256) keeps
// Montgomery twiddles.
template <class Fr>
struct ShoupTw {
  Fr w, wq;
};
template <class Fr>
struct NttTw {
  using type = Fr;
};
template <>
struct NttTw<Bn254Fr> {
  using type = ShoupTw<Bn254Fr>;
};
template <class Fr>
__device__ __forceinline__ Fr tw_mul(const Fr& x, const Fr& w) {
  return x * w;
}
template <class Fr>
__device__ __forceinline__ Fr tw_mul(const Fr& x, const ShoupTw<Fr>& t) {
  return x.mul_shoup(t.w, t.wq);
}

template <class Fr>
struct PassArgs {
  uint32_t L, s0, k, log_m, final_pass, mode, pow_bits;
  const Fr* load_lo;
  const Fr* load_hi;
  const Fr* store_lo;
  const Fr* store_hi;
  Fr scale;
  // four-step exchange (kStoreTw4: the forward stage 1's last pass; kLoadTw4:
  // the inverse stage 2's first pass): element k of batch entry b (the local
  // column c_l) times w_N^(+-(c0 + b) k), at its packed send / recv position
  FourStepTw<Fr> fs;
  // single-pass transforms smaller than a tile: 2^pack batch entries per
  // workgroup, set m = entry (blockIdx.y << pack) + m (0: one entry per blockIdx.y)
  uint32_t pack;
};

// The exchange layout of the fused stages: chunk h (n/G^2 elements, to / from
// rank h) holds [k1_l][c_l], row-major -- so the row NTTs read (forward
// stage 2) and write (inverse stage 1) Cg-element runs and need no transpose.
// Column side: element k1 of local column c_l at (h Rg + k1_l) Cg + c_l =
// k1 Cg + c_l (h = k1 >> log_rg).  (The unfused round-4 stages keep
// twiddle_exchange_kernel's [c_l][k1_l] chunks and the transposes.)
template <class Fr>
__device__ __forceinline__ size_t fs_packed(const FourStepTw<Fr>& f, uint32_t k1, uint32_t c_l) {
  return ((size_t)k1 << f.log_cg) + c_l;
}
// Row side: element c (column, c = g Cg + c_l) of local row j at (g Rg + j) Cg + c_l
template <class Fr>
__device__ __forceinline__ size_t xch_pos(const FourStepTw<Fr>& f, uint32_t c, uint32_t j) {
  return ((((size_t)(c >> f.log_cg) << f.log_rg) + j) << f.log_cg) + (c & ((1u << f.log_cg) - 1));
}
// w_N^((c0 + c_l) k1) from the two-level power tables of the four-step's root
template <class Fr>
__device__ __forceinline__ Fr fs_twiddle(const FourStepTw<Fr>& f, uint32_t k1, uint32_t c_l) {
  const uint64_t e = ((uint64_t)(f.c0 + c_l) * k1) & ((uint64_t(1) << f.log_n) - 1);
  return f.lo[e & ((1u << f.bits) - 1)] * f.hi[e >> f.bits];
}

__device__ __forceinline__ uint32_t bitrev(uint32_t x, uint32_t bits) {
  return bits == 0 ? 0u : (__brev(x) >> (32 - bits));
}

// One pass of k DIF stages (s0 .. s0+k-1) over M sets of 2^k elements held in
// LDS.  Non-final passes are in place (each workgroup reads and writes the
// same positions); the final pass (s0 + k == L) writes natural order through
// the bit-reversal permutation, M bit-reversed-consecutive sets per workgroup
// so every store row is M contiguous elements.
// R DIF stages (t .. t+R-1 of the pass) on groups of 2^R elements held in
// registers.  Group g covers set m = g mod M and the positions
// a0 + j q (j < 2^R, q = 2^(k-t-R)); stage t+u pairs j with j + 2^(R-1-u).
// Twiddle of the butterfly whose low element has global index i at global
// stage s: w_s^(i mod 2^(L-s-1)) (the reference's Radix2TwiddleCache row s).
// kLast: the transform's last R stages (final pass, t + R == k).
template <int R, bool kLast, bool kPrefetch, class Fr, class Tw, class IndexFn>
__device__ __forceinline__ void radix_step(Fr* __restrict__ lds, const Tw* __restrict__ tw, const PassArgs<Fr>& a,
                                           uint32_t t, IndexFn index) {
  constexpr int E = 1 << R;
  const uint32_t log_m = a.log_m, M = 1u << log_m;
  const uint32_t n = 1u << a.L;
  const uint32_t groups = (M << a.k) >> R;
  const uint32_t qlog = a.k - t - R;
  for (uint32_t g = threadIdx.x; g < groups; g += kBlock) {
    const uint32_t m = g & (M - 1);
    const uint32_t rr = g >> log_m;
    const uint32_t off = rr & ((1u << qlog) - 1);
    const uint32_t a0 = ((rr >> qlog) << (qlog + R)) + off;
    // the step's twiddles first: their global loads overlap the LDS reads
    // and the first butterflies instead of stalling each product
    Tw wv[R][E / 2];
    if constexpr (!kLast && kPrefetch) {
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const uint32_t st = a.s0 + t + u;
        const uint32_t gap_mask = (1u << (a.L - st - 1)) - 1;
        const Tw* tws = tw + (n - (n >> st));
        const int half = E >> (u + 1);
        int c = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          if (j & half) continue;
          wv[u][c++] = tws[index(a0 + ((uint32_t)j << qlog), m) & gap_mask];
        }
      }
    }
    Fr x[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = lds[((a0 + ((uint32_t)j << qlog)) << log_m) + m];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const uint32_t st = a.s0 + t + u;
      const Tw* tws = tw + (n - (n >> st));
      const int half = E >> (u + 1);
      int c = 0;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (j & half) continue;
        const Fr lo = x[j], hi = x[j + half];
        // ButterflyFnInOut: lo = lo + hi; hi = (lo - hi) * w
        x[j] = lo + hi;
        if constexpr (kLast) {
          // the transform's last R stages: the twiddle index is j mod 2^(R-1-u)
          // (a0 and the set base are multiples of 2^R), known at compile time;
          // index 0 is w = 1 -- the whole last stage and half the one before
          const uint32_t idx = (uint32_t)j & ((1u << (R - 1 - u)) - 1);
          x[j + half] = idx ? tw_mul(lo.sub_unreduced(hi), tws[idx]) : (lo - hi);
        } else {
          // twiddles are canonical, so lo - hi + 2p needs no borrow test
          if constexpr (kPrefetch) {
            x[j + half] = tw_mul(lo.sub_unreduced(hi), wv[u][c++]);
          } else {
            const uint32_t gap_mask = (1u << (a.L - st - 1)) - 1;
            x[j + half] = tw_mul(lo.sub_unreduced(hi), tws[index(a0 + ((uint32_t)j << qlog), m) & gap_mask]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < E; ++j) lds[((a0 + ((uint32_t)j << qlog)) << log_m) + m] = x[j];
  }
}

template <class Fr, class Tw, int MaxR, bool kPrefetch = true, int kWaves = 1>
__global__ __launch_bounds__(kBlock, kWaves) void dif_pass_kernel(const Fr* __restrict__ in, Fr* __restrict__ out,
                                                          const Tw* __restrict__ tw, PassArgs<Fr> a) {
  extern __shared__ uint4 smem_raw[];
  Fr* lds = reinterpret_cast<Fr*>(smem_raw);
  const uint32_t L = a.L, k = a.k, log_m = a.log_m;
  const uint32_t M = 1u << log_m;
  const uint32_t elems = M << k;
  const uint32_t b = blockIdx.x;
  // batch of independent contiguous transforms (the packed four-step
  // layouts address the whole buffer themselves); with a.pack the workgroup's
  // sets are 2^pack whole transforms, entries ybase + m
  const uint32_t pk = a.pack, ybase = blockIdx.y << pk;
  if (!(a.mode & (kLoadTw4 | kLoadXch))) in += (size_t)ybase << L;
  if (!(a.mode & (kStoreTw4 | kStoreXch))) out += (size_t)ybase << L;

  // index(mid, m) of element m of the block's set, position mid in the set
  uint32_t hi_shift = L - a.s0;            // set stride in the hi dimension
  uint32_t mid_shift = L - a.s0 - k;       // stride between set members
  uint32_t hi = 0, lo_base = 0, r0 = 0;
  if (!a.final_pass) {
    uint32_t lo_blocks = (1u << mid_shift) >> log_m;
    hi = b / lo_blocks;
    lo_base = (b - hi * lo_blocks) << log_m;
  } else {
    r0 = b << log_m;
  }
  auto index = [&](uint32_t mid, uint32_t m) -> uint32_t {
    if (!a.final_pass) return (hi << hi_shift) + (mid << mid_shift) + lo_base + m;
    uint32_t h = bitrev(r0 + m, L - k);
    return (h << k) + mid;
  };

  // ---- load ----
  for (uint32_t e = threadIdx.x; e < elems; e += kBlock) {
    uint32_t mid = e >> log_m, m = e & (M - 1);
    uint32_t i = index(mid, m);
    const uint32_t ent = pk ? m : 0u;
    Fr v;
    if (a.mode & kLoadTw4) {
      v = in[fs_packed(a.fs, i, ybase + ent)] * fs_twiddle(a.fs, i, ybase + ent);
    } else if (a.mode & kLoadXch) {
      v = in[xch_pos(a.fs, i, ybase + ent)];
    } else {
      v = in[((size_t)ent << L) + i];
      if (a.mode & kLoadCoset) v = v * (a.load_lo[i & ((1u << a.pow_bits) - 1)] * a.load_hi[i >> a.pow_bits]);
    }
    lds[e] = v;
  }
  __syncthreads();

  // ---- k butterfly stages, up to MaxR per LDS round trip ----
  // A step of R stages loads 2^R elements of one set into registers, runs
  // the R * 2^(R-1) butterflies there (2^(R-1) independent ones per stage,
  // which the scheduler interleaves) and writes them back: one LDS round
  // trip and one barrier per R stages instead of per stage.
  for (uint32_t t = 0; t < k;) {
    const uint32_t R = min((uint32_t)MaxR, k - t);
    const bool last = a.final_pass && t + R == k;
    if (MaxR >= 3 && R == 3) {
      if (last) radix_step<3, true, kPrefetch>(lds, tw, a, t, index);
      else radix_step<3, false, kPrefetch>(lds, tw, a, t, index);
    } else if (MaxR >= 2 && R == 2) {
      if (last) radix_step<2, true, kPrefetch>(lds, tw, a, t, index);
      else radix_step<2, false, kPrefetch>(lds, tw, a, t, index);
    } else {
      if (last) radix_step<1, true, kPrefetch>(lds, tw, a, t, index);
      else radix_step<1, false, kPrefetch>(lds, tw, a, t, index);
    }
    t += R;
    __syncthreads();
  }

  // ---- store ----
  if (!a.final_pass) {
    for (uint32_t e = threadIdx.x; e < elems; e += kBlock) {
      uint32_t mid = e >> log_m, m = e & (M - 1);
      out[index(mid, m)] = lds[e];
    }
  } else {
    for (uint32_t e = threadIdx.x; e < elems; e += kBlock) {
      uint32_t q = e >> log_m, m = e & (M - 1);
      uint32_t mid = bitrev(q, k);
      Fr v = lds[(mid << log_m) + m];
      const uint32_t o = pk ? q : (q << (L - k)) + r0 + m, ent = pk ? m : 0u;
      if (a.mode & kStoreCoset) v = v * (a.store_lo[o & ((1u << a.pow_bits) - 1)] * a.store_hi[o >> a.pow_bits]);
      else if (a.mode & kStoreScale) v = v * a.scale;
      if (a.mode & kStoreTw4) out[fs_packed(a.fs, o, ybase + ent)] = (v * fs_twiddle(a.fs, o, ybase + ent)).canonical();
      else if (a.mode & kStoreXch) out[xch_pos(a.fs, o, ybase + ent)] = v.canonical();
      else out[((size_t)ent << L) + o] = v.canonical();
    }
  }
}

}  // namespace

}  // namespace tachyon_amd::ntt
