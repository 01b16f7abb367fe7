// The BN254 Fr NTT pass over 9 x 29-bit limbs: dif29_pass_kernel and the
// kernel that builds its twiddle tables.  Device code of ntt.hip's translation
// unit: included there only, after ntt_pass32.h (PassArgs, the pass modes, the
// four-step helpers and bitrev are shared with the 32-bit pass).
#pragma once
#include "../field/fr29.h"
#include "ntt_pass32.h"

namespace tachyon_amd::ntt {

namespace {

// ---------------------------------------------------------------------------
// BN254 Fr passes over 9 x 29-bit limbs (field/fr29.h): the same DIF network,
// pass plan, index maps, bit reversal and fused scalings as dif_pass_kernel,
// with the butterflies of fr29::radix4 / radix2 (carry-free products, limb-wise
// sums and differences).  Elements between passes are 36-byte F29 (normalized,
// < 8p); the first pass reads the 32-byte Montgomery input, the final pass
// writes canonical 32-byte values.  LDS holds the elements as 9 limb planes
// of kMaxLdsElems words (a plane stride fixed at compile time: one ds_read_b32
// per limb with an immediate offset).  Twiddles: R'-form (36 B) in the first
// pass, whose stage tables stream from HBM; Shoup (72 B) in the later ones.
using fr29::F29;
template <class TwT>
struct Tw29Table {
  const TwT* tw;  // entry of (stage s, index j) at tw[(n - (n >> s)) - off + j]
  uint32_t off;
};

// kSwz: positions XOR-swizzled so that the 32-lane groups of a ds_read_b32 /
// ds_write_b32 (bank = word mod 32) hit 32 distinct banks in every register
// step of the 8-stage, 4-set passes (2^24: qlog = 6, 4, 2, 0): bit 2 ^= bit 5,
// bits 3, 4 ^= bit 6.  Without it the qlog = 2 / 0 steps are 2- / 4-way
// conflicted on all 72 LDS accesses of a group.
template <bool kSwz>
__device__ __forceinline__ uint32_t swz29(uint32_t p) {
  if constexpr (kSwz) return p ^ ((p >> 3) & 4u) ^ (((p >> 6) & 1u) * 0x18u);
  else return p;
}
template <bool kSwz>
__device__ __forceinline__ F29 lds29_load(const uint32_t* __restrict__ lds, uint32_t pos) {
  F29 v;
  pos = swz29<kSwz>(pos);
#pragma unroll
  for (int i = 0; i < 9; ++i) v.l[i] = lds[i * kMaxLdsElems + pos];
  return v;
}
template <bool kSwz>
__device__ __forceinline__ void lds29_store(uint32_t* __restrict__ lds, uint32_t pos, const F29& v) {
  pos = swz29<kSwz>(pos);
#pragma unroll
  for (int i = 0; i < 9; ++i) lds[i * kMaxLdsElems + pos] = v.l[i];
}

template <int R, bool kLast, bool kSwz, class TwT, class IndexFn>
__device__ __forceinline__ void radix29_step(uint32_t* __restrict__ lds, Tw29Table<TwT> tt,
                                             const PassArgs<Bn254Fr>& a, uint32_t t, IndexFn index) {
  constexpr int E = 1 << R;
  const uint32_t log_m = a.log_m, M = 1u << log_m;
  const uint32_t n = 1u << a.L;
  const uint32_t groups = (M << a.k) >> R;
  const uint32_t qlog = a.k - t - R;
  const uint32_t st = a.s0 + t;
  const TwT* twA = tt.tw + ((n - (n >> st)) - tt.off);
  const uint32_t gapA = (1u << (a.L - st - 1)) - 1;
  for (uint32_t g = threadIdx.x; g < groups; g += kBlock) {
    const uint32_t m = g & (M - 1);
    const uint32_t rr = g >> log_m;
    const uint32_t off = rr & ((1u << qlog) - 1);
    const uint32_t a0 = ((rr >> qlog) << (qlog + R)) + off;
    if constexpr (R == 2) {
      // twiddles first: their loads overlap the LDS reads
      TwT tA0, tA1, tB0, tB1;
      if constexpr (kLast) {
        tA1 = twA[1];  // stage L - 2 has the two entries {1, w_4}; everything else is 1
      } else {
        const TwT* twB = tt.tw + ((n - (n >> (st + 1))) - tt.off);
        const uint32_t gapB = (1u << (a.L - st - 2)) - 1;
        tA0 = twA[index(a0, m) & gapA];
        tA1 = twA[index(a0 + (1u << qlog), m) & gapA];
        tB0 = twB[index(a0, m) & gapB];
        tB1 = twB[index(a0 + (2u << qlog), m) & gapB];
      }
      F29 x[4];
#pragma unroll
      for (int j = 0; j < E; ++j) x[j] = lds29_load<kSwz>(lds, ((a0 + ((uint32_t)j << qlog)) << log_m) + m);
      if constexpr (kLast) fr29::radix4_last(x, tA1);
      else fr29::radix4(x, tA0, tA1, tB0, tB1);
#pragma unroll
      for (int j = 0; j < E; ++j) lds29_store<kSwz>(lds, ((a0 + ((uint32_t)j << qlog)) << log_m) + m, x[j]);
    } else {
      TwT tA;
      if constexpr (!kLast) tA = twA[index(a0, m) & gapA];
      F29 x[2];
#pragma unroll
      for (int j = 0; j < E; ++j) x[j] = lds29_load<kSwz>(lds, ((a0 + ((uint32_t)j << qlog)) << log_m) + m);
      if constexpr (kLast) fr29::radix2_last(x);
      else fr29::radix2(x, tA);
#pragma unroll
      for (int j = 0; j < E; ++j) lds29_store<kSwz>(lds, ((a0 + ((uint32_t)j << qlog)) << log_m) + m, x[j]);
    }
  }
}

// kFirst: the input is the 32-byte Montgomery array (the transform's first
// pass, R'-form twiddles); otherwise 36-byte F29 from the previous pass.
template <bool kFirst, bool kSwz, class TwT>
__global__ __launch_bounds__(kBlock) void dif29_pass_kernel(const void* __restrict__ in_v, void* __restrict__ out_v,
                                                            Tw29Table<TwT> tt, PassArgs<Bn254Fr> a) {
  __shared__ uint32_t lds[9 * kMaxLdsElems];
  const uint32_t L = a.L, k = a.k, log_m = a.log_m;
  const uint32_t M = 1u << log_m;
  const uint32_t elems = M << k;
  const uint32_t b = blockIdx.x;
  uint32_t hi_shift = L - a.s0;
  uint32_t mid_shift = L - a.s0 - k;
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
  // (a.pack: the workgroup's sets are 2^pack whole transforms, entries ybase + m)
  const uint32_t pk = a.pack, ybase = blockIdx.y << pk;
  const size_t batch_off = (size_t)ybase << L;
  for (uint32_t e = threadIdx.x; e < elems; e += kBlock) {
    const uint32_t mid = e >> log_m, m = e & (M - 1);
    const uint32_t i = index(mid, m);
    const uint32_t ent = pk ? m : 0u;
    F29 v;
    if constexpr (kFirst) {
      Bn254Fr x;
      if ((a.mode & kLoadTw4) && a.fs.tab29) {  // the precomputed R'-form twiddle: one product
        const Bn254Fr raw = static_cast<const Bn254Fr*>(in_v)[fs_packed(a.fs, i, ybase + ent)];
        const auto* t29 = static_cast<const fr29::TwMont29*>(a.fs.tab29);
        v = fr29::tw_prod(fr29::from_words(raw.v), t29[((size_t)(ybase + ent) << a.fs.log_r) + i]);
        lds29_store<kSwz>(lds, e, v);
        continue;
      }
      if (a.mode & kLoadTw4) {
        x = static_cast<const Bn254Fr*>(in_v)[fs_packed(a.fs, i, ybase + ent)] * fs_twiddle(a.fs, i, ybase + ent);
      } else if (a.mode & kLoadXch) {
        x = static_cast<const Bn254Fr*>(in_v)[xch_pos(a.fs, i, ybase + ent)];
      } else {
        x = static_cast<const Bn254Fr*>(in_v)[batch_off + ((size_t)ent << L) + i];
        if (a.mode & kLoadCoset) x = x * (a.load_lo[i & ((1u << a.pow_bits) - 1)] * a.load_hi[i >> a.pow_bits]);
      }
      v = fr29::from_words(x.v);
    } else {
      v = static_cast<const F29*>(in_v)[batch_off + ((size_t)ent << L) + i];
    }
    lds29_store<kSwz>(lds, e, v);
  }
  __syncthreads();

  for (uint32_t t = 0; t < k;) {
    const uint32_t R = min(2u, k - t);
    const bool last = a.final_pass && t + R == k;
    if (R == 2) {
      if (last) radix29_step<2, true, kSwz>(lds, tt, a, t, index);
      else radix29_step<2, false, kSwz>(lds, tt, a, t, index);
    } else {
      if (last) radix29_step<1, true, kSwz>(lds, tt, a, t, index);
      else radix29_step<1, false, kSwz>(lds, tt, a, t, index);
    }
    t += R;
    __syncthreads();
  }

  // ---- store ----
  if (!a.final_pass) {
    F29* out = static_cast<F29*>(out_v) + batch_off;
    for (uint32_t e = threadIdx.x; e < elems; e += kBlock) {
      const uint32_t mid = e >> log_m, m = e & (M - 1);
      out[index(mid, m)] = lds29_load<kSwz>(lds, e);
    }
  } else {
    Bn254Fr* out = static_cast<Bn254Fr*>(out_v) + ((a.mode & (kStoreTw4 | kStoreXch)) ? 0 : batch_off);
    for (uint32_t e = threadIdx.x; e < elems; e += kBlock) {
      const uint32_t q = e >> log_m, m = e & (M - 1);
      const uint32_t mid = bitrev(q, k);
      Bn254Fr v;
      const uint32_t o = pk ? q : (q << (L - k)) + r0 + m, ent = pk ? m : 0u;
      if ((a.mode & kStoreTw4) && a.fs.tab29) {  // the precomputed R'-form twiddle: one product
        const auto* t29 = static_cast<const fr29::TwMont29*>(a.fs.tab29);
        const F29 y = fr29::tw_prod(lds29_load<kSwz>(lds, (mid << log_m) + m),
                                    t29[((size_t)(ybase + ent) << a.fs.log_r) + o]);
        fr29::to_canonical_words(y, v.v);
        out[fs_packed(a.fs, o, ybase + ent)] = v;
        continue;
      }
      fr29::to_canonical_words(lds29_load<kSwz>(lds, (mid << log_m) + m), v.v);
      if (a.mode & kStoreCoset) v = (v * (a.store_lo[o & ((1u << a.pow_bits) - 1)] * a.store_hi[o >> a.pow_bits])).canonical();
      else if (a.mode & kStoreScale) v = (v * a.scale).canonical();
      if (a.mode & kStoreTw4) out[fs_packed(a.fs, o, ybase + ent)] = (v * fs_twiddle(a.fs, o, ybase + ent)).canonical();
      else if (a.mode & kStoreXch) out[xch_pos(a.fs, o, ybase + ent)] = v;
      else out[((size_t)ent << L) + o] = v;
    }
  }
}

// Montgomery twiddles (canonical w 2^256 mod p) -> the 29-bit tables: entries
// [0, split) R'-form (w 2^261 mod p = 32 W mod p), entries [split, count)
// Shoup {w, floor(w 2^261 / p)} with floor(w 2^261 / p) = 32 floor(w 2^256 /
// p) + floor(32 W / p) (W = w 2^256 mod p, the Montgomery entry).
__global__ __launch_bounds__(kBlock) void tw29_table_kernel(fr29::TwMont29* __restrict__ mont29,
                                                            fr29::TwShoup29* __restrict__ shoup29,
                                                            const Bn254Fr* __restrict__ in, uint32_t split,
                                                            uint32_t count) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= count) return;
  const Bn254Fr W = in[j].canonical();
  if (j < split) {
    Bn254Fr x = W;
#pragma unroll
    for (int i = 0; i < 5; ++i) x = (x + x).canonical();
    mont29[j].w = fr29::from_words(x.v);
  } else {
    const Bn254Fr w = W.from_mont();
    const Bn254Fr q32 = Bn254Fr::shoup_quotient(w);
    // t = floor(32 W / p): five doublings of W (< p, so 2r < 2p < 2^256),
    // each followed by a subtraction of p when 2r >= p (one quotient bit)
    uint32_t t = 0;
    uint32_t r[8];
    for (int i = 0; i < 8; ++i) r[i] = W.v[i];
    for (int bit = 0; bit < 5; ++bit) {
      uint32_t c = 0;
      for (int i = 0; i < 8; ++i) {
        const uint32_t nc = r[i] >> 31;
        r[i] = (r[i] << 1) | c;
        c = nc;
      }
      uint32_t d[8], borrow = 0;
      for (int i = 0; i < 8; ++i) {
        const uint64_t s = (uint64_t)r[i] - fr29::kPWords[i] - borrow;
        d[i] = (uint32_t)s;
        borrow = (uint32_t)(s >> 63);
      }
      t = 2 * t + (borrow ? 0u : 1u);
      if (!borrow)
        for (int i = 0; i < 8; ++i) r[i] = d[i];
    }
    fr29::TwShoup29 e;
    e.w = fr29::from_words(w.v);
    e.wq = f29::shl5_repack(q32.v);
    e.wq.l[0] |= t;  // the low 5 bits of 32 q32 are zero
    shoup29[j - split] = e;
  }
}

}  // namespace

}  // namespace tachyon_amd::ntt
