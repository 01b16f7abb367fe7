// MSM stage 3, bucket accumulation: the one-lane, limb-field and lane-pair kernels
// (part of msm_impl.h).
#pragma once

namespace tachyon_amd::msm {
namespace detail {
namespace {  // internal linkage: every per-curve TU gets its own copy

// ---------------------------------------------------------------------------
// Load-balanced bucket accumulation.
//
// The per-window sorted (bucket, point) lists are one array of W*n entries,
// ordered by (window, bucket).  Thread t owns entries [t*K, (t+1)*K) -- every
// lane runs exactly K mixed additions whatever the bucket sizes (a bucket per
// lane left lanes idle for the longest bucket of their wave).  A run of equal
// buckets inside the range is summed with madd-2008-s (XYZZ += +-affine):
//   * a run that starts and ends inside the range is that bucket's whole sum
//     -> stored straight to bucket_sum[b] (the only writer);
//   * the first run, if the bucket started in an earlier thread ("head"), and
//     the last run, if it continues into the next thread ("tail"), go to
//     pieces[2t] / pieces[2t+1] and are joined by the chain kernels below.
// Minimum waves per SIMD of the point-arithmetic kernels.  Left alone, the
// scheduler interleaves the three Karatsuba products of an Fq2 multiply and
// the G2 kernels land at 256+ VGPRs = one wave per SIMD; capping them at two
// waves (a little scratch) made the BN254 G2 2^24 accumulation 89 -> 61 ms
// and BLS12-381 G2 212 -> 174 ms.
template <class Curve>
struct AccWaves {
  static constexpr int value = 1;
};
// BLS12-381 G1: two waves per SIMD for the 28-bit reductions (the window
// segment kernel then spills 348 B per lane, but at one wave it ran 1664 waves
// of dependent products on 1024 SIMDs): 2^24 reduction 5.5 -> 5.0 ms
// (profiles/r06p/ab_bls_g1_reduction_waves.log)
#ifndef TACHYON_BLS_G1_RED_WAVES
#define TACHYON_BLS_G1_RED_WAVES 2
#endif
template <>
struct AccWaves<Bls381G1> {
  static constexpr int value = TACHYON_BLS_G1_RED_WAVES;
};
template <>
struct AccWaves<Bn254G2> {
  static constexpr int value = 2;
};
template <>
struct AccWaves<Bls381G2> {
  static constexpr int value = 2;
};
// The identity accumulator as a flag (see seg_acc_kernel): every curve but
// BN254 G2, whose inline Fq2 products leave no registers for the extra live
// state (2^20 accumulation 5.30 -> 5.59 ms with it; BLS12-381 G2, whose Fq
// products are calls, 23.4 -> 21.3 ms at 2^21).  The 2-wave cap above
// measured best for both G2 kernels against 1 and 3 waves.
template <class Curve>
struct AccFlag {
  static constexpr bool value = true;
};
template <>
struct AccFlag<Bn254G2> {
  static constexpr bool value = false;
};

template <class Curve>
__global__ __launch_bounds__(kBlock, AccWaves<Curve>::value) void seg_acc_kernel(const Affine<typename Curve::F>* __restrict__ bases,
                                                         const uint64_t* __restrict__ ents, uint32_t c,
                                                         uint64_t gbeg, uint64_t gend, uint64_t tbase,
                                                         uint32_t K, uint32_t idx_mask,
                                                         XYZZ<typename Curve::F>* __restrict__ bucket_sum,
                                                         XYZZ<typename Curve::F>* __restrict__ pieces,
                                                         uint32_t* __restrict__ tflags,
                                                         uint32_t* __restrict__ tlast) {
  using F = typename HotOf<typename Curve::F>::type;  // inline products in this kernel (same layout)
  const Affine<F>* __restrict__ hbases = reinterpret_cast<const Affine<F>*>(bases);
  XYZZ<F>* __restrict__ hsum = reinterpret_cast<XYZZ<F>*>(bucket_sum);
  XYZZ<F>* __restrict__ hpieces = reinterpret_cast<XYZZ<F>*>(pieces);
  const uint64_t tl = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t g0 = gbeg + tl * K;
  if (g0 >= gend) return;
  const uint64_t g1 = min(g0 + K, gend);
  const uint64_t t = tbase + tl;  // global thread slot (pieces/flags are in entry order)
  // neighbours outside this launch's entry range belong to other windows
  // (possibly not sorted yet): they never share a bucket
  const uint32_t prev_b = g0 > gbeg ? bucket_of_key(entry_key(ents[g0 - 1]), c) : kNoBucket;
  const uint32_t next_b = (g1 < gend) ? bucket_of_key(entry_key(ents[g1]), c) : kNoBucket;

  uint32_t flags = 0, runs = 0, cur = kNoBucket;
  XYZZ<F> acc = XYZZ<F>::zero();
  // The identity accumulator is a flag, not a test of zz: a run starts from
  // its first non-identity base (no madd), identity bases (0, 0) -- canonical
  // input, so a plain limb OR -- add nothing, and madd_nz reports the rare
  // cancellation P = -acc.  Signed digits negate y as p - y by limb selects.
  // (AccFlag: all curves but BN254 G2)
  constexpr bool kFlag = AccFlag<Curve>::value;
  bool acc_zero = true;
  // two-deep software pipeline: the entry of g+2 and the base of g+1 are in
  // flight while the madd for g runs (one-word and BLS12-381 Fq fields).  (A 3-deep pipeline and >= 4 waves per
  // SIMD at 128 VGPRs measured the same for BN254 G1 -- 72.4 / 72.2 vs 72.2
  // ms at 2^26 -- the kernel is issue-bound; the array-rotated 3-deep form
  // also cost the BLS12-381 G2 kernel 8 % in scratch traffic.)
  // Fq2 (G2) kernels load each base at its own iteration: the prefetched
  // next point (64 / 96 words) costs them spills at the 2-wave register cap
  // (BLS12-381 G2 2^21 accumulation 25.7 -> 23.6 ms, BN254 G2 2^20 5.55 ->
  // 5.42 without it; the second wave covers the gather latency)
  constexpr bool kPrefetchBase = sizeof(F) <= 48;
  uint64_t e0 = ents[g0];
  uint64_t e1 = (g0 + 1 < g1) ? ents[g0 + 1] : 0;
  Affine<F> P;
  if constexpr (kPrefetchBase) P = hbases[entry_val(e0) & idx_mask];
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t e2 = (g + 2 < g1) ? ents[g + 2] : 0;
    Affine<F> Pn;
    if constexpr (kPrefetchBase) Pn = hbases[entry_val(e1) & idx_mask];
    else P = hbases[entry_val(e0) & idx_mask];
    const uint32_t k0 = entry_key(e0), v0 = entry_val(e0);
    const uint32_t b = bucket_of_key(k0, c);
    if (b != kNoBucket) {
      if (b != cur) {
        if (cur != kNoBucket) {  // close a run that is not the last one
          if constexpr (kFlag)
            if (acc_zero) acc = XYZZ<F>::zero();
          if (runs == 1 && cur == prev_b) { hpieces[2 * t] = acc; flags |= kHead; }
          else hsum[cur] = acc;
        }
        cur = b;
        ++runs;
        if constexpr (kFlag) acc_zero = true;
        else acc = XYZZ<F>::zero();
      }
      if constexpr (kFlag) {
        if (!P.is_zero_canonical()) {
          P.y = P.y.cond_neg_canonical(v0 & kSignBit);
          if (acc_zero) {
            acc = XYZZ<F>{P.x, P.y, F::one(), F::one()};
            acc_zero = false;
          } else {
            acc = acc.madd_nz(P, &acc_zero);
          }
        }
      } else {
        // BN254 G2: the generic identity-aware madd and no flag (AccFlag)
        if ((v0 & kSignBit) && !P.is_zero()) P.y = -P.y;
        acc = acc.madd(P);
      }
    }
    e0 = e1;
    e1 = e2;
    if constexpr (kPrefetchBase) P = Pn;
  }
  if constexpr (kFlag)
    if (acc_zero) acc = XYZZ<F>::zero();
  if (cur != kNoBucket) {  // the last run
    const bool head = runs == 1 && cur == prev_b;
    const bool tail = cur == next_b;
    if (head) { hpieces[2 * t] = acc; flags |= kHead; }
    if (tail) flags |= kTail;
    if (tail && !head) hpieces[2 * t + 1] = acc;
    if (!head && !tail) hsum[cur] = acc;
  }
  if (runs <= 1) flags |= kSingle;
  // absent pieces are the identity so every chain sums a contiguous range
  if (!(flags & kHead)) hpieces[2 * t] = XYZZ<F>::zero();
  const bool through = (flags & kHead) && (flags & kTail) && (flags & kSingle);
  if (!(flags & kTail) || through) hpieces[2 * t + 1] = XYZZ<F>::zero();
  tflags[t] = flags;
  tlast[t] = cur;
}

// ---------------------------------------------------------------------------
// BN254 G1 accumulation over the carry-free 29-bit-limb field (field/f29.h).
// The same load-balanced run logic as seg_acc_kernel; the accumulator lives
// in R' = 2^261 form (Raw stores) -- the point formulas and their value
// bounds are in msm/acc29.h.
namespace acc29 {
using namespace ::tachyon_amd::f29;
using namespace ::tachyon_amd::msm::acc29_core;  // Acc, from_shifted, madd, add, dbl (msm/acc29.h)
__device__ __forceinline__ XYZZ<Bn254Fq> to_xyzz(const Acc& a) {
  XYZZ<Bn254Fq> r;
  to32(a.x, r.x.v);
  to32(a.y, r.y.v);
  to32(a.zz, r.zz.v);
  to32(a.zzz, r.zzz.v);
  return r;
}
// P == acc: through the R-form doubling (rare).  Inline: an out-of-line call
// takes the accumulator's address and the compiler then keeps it in scratch
// for the whole loop (a 288-byte scratch round trip per madd: 2^26 82.7 ms)
__device__ __forceinline__ Acc dbl_slow(const Acc& a) {
  using HF = HotFp<Bn254Fq>;
  XYZZ<Bn254Fq> s = to_xyzz(a);
  XYZZ<HF> h{s.x, s.y, s.zz, s.zzz};
  h = h.dbl();
  return {from32(h.x.v), from32(h.y.v), from32(h.zz.v), from32(h.zzz.v)};
}



// A reduction operand with its identity flag, to and from the R-form arrays
struct Pt {
  Acc a;
  bool zero;
};
__device__ __forceinline__ Pt load_pt(const XYZZ<Bn254Fq>* __restrict__ p, size_t i) {
  const XYZZ<Bn254Fq> q = p[i];
  if (q.is_zero()) return {Acc{}, true};
  return {{from32(q.x.v), from32(q.y.v), from32(q.zz.v), from32(q.zzz.v)}, false};
}
__device__ __forceinline__ void store_pt(XYZZ<Bn254Fq>* __restrict__ p, size_t i, const Pt& v) {
  p[i] = v.zero ? XYZZ<Bn254Fq>::zero() : to_xyzz(v.a);
}
__device__ __forceinline__ Pt add(const Pt& a, const Pt& b) {
  if (a.zero) return b;
  if (b.zero) return a;
  int special = 0;
  const Acc s = add(a.a, b.a, &special);
  if (special == 1) return {Acc{}, true};
  return {special == 2 ? dbl(a.a) : s, false};
}
// A bucket or piece as the 29-bit accumulation leaves it (R' form, 4 x 9
// limbs, 144 B; all-zero limbs = the identity): the accumulation's run-end
// stores skip the four R-form conversions (they run in the loop's divergent
// branch whenever any lane of the wave changes bucket) and the 29-bit
// reductions read it without converting.
struct alignas(16) Raw {
  F29 x, y, zz, zzz;
};
// the identity is zz = 0 alone (load_raw tests zz; x, y, zzz are not read
// then): one 9-limb select instead of four in the run-end stores
__device__ __forceinline__ Raw raw_of(const Acc& a, bool zero) {
  Raw r{a.x, a.y, a.zz, a.zzz};
#pragma unroll
  for (int k = 0; k < 9; ++k) r.zz.l[k] = zero ? 0u : a.zz.l[k];
  return r;
}
__device__ __forceinline__ Pt load_raw(const void* __restrict__ p, size_t i) {
  const Raw r = static_cast<const Raw*>(p)[i];
  uint32_t nz = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) nz |= r.zz.l[k];
  return {{r.x, r.y, r.zz, r.zzz}, nz == 0};
}
__device__ __forceinline__ void store_raw(void* __restrict__ p, size_t i, const Pt& v) {
  static_cast<Raw*>(p)[i] = raw_of(v.a, v.zero);
}

// m P for a small m (double-and-add from the top bit)
__device__ __forceinline__ Pt small_mul(const Pt& P, uint32_t m) {
  if (m == 0 || P.zero) return {Acc{}, true};
  Pt r = P;
  for (int bit = 30 - __builtin_clz(m); bit >= 0; --bit) {
    r.a = dbl(r.a);  // (no point of this prime-order group doubles to the identity)
    if ((m >> bit) & 1) r = add(r, P);
  }
  return r;
}
}  // namespace acc29

// The field policies of seg_acc_limb_body: BN254 G1 over the 9 x 29-bit field
// (Raw 144-byte stores, the rare doubling through the R-form FIPS field) and
// BLS12-381 G1 over the 14 x 28-bit field (R-form stores for the FIPS
// reductions, the doubling in 28-bit limbs).
struct Pol29 {
  using Fq = Bn254Fq;
  using F = f29::F29;
  using Acc = acc29::Acc;
  using Raw = acc29::Raw;
  static __device__ __forceinline__ F shift_repack(const uint32_t* w) { return f29::shl5_repack(w); }
  // the base's y for a digit of sign `neg`: y~ << 5 (< 32p), negated in the
  // 29-bit limbs as 33p - y~ << 5 (kK33's raised limbs: no borrows; the value
  // stays < 33p, which madd's bounds allow) -- 9 subtractions and 9 selects
  // instead of a borrow chain over the canonical 32-bit words
  static __device__ __forceinline__ F repack_y(const Fq& y, uint32_t neg) {
    F r = f29::shl5_repack(y.v);
    const F m = f29::ksub(f29::kK33, r);
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = neg ? m.l[i] : r.l[i];
    return r;
  }
  static __device__ __forceinline__ Acc from_shifted(const F& x, const F& y) { return acc29::from_shifted(x, y); }
  static __device__ __forceinline__ Acc madd(const Acc& a, const F& x, const F& y, int* sp) {
    return acc29::madd(a, x, y, sp);
  }
  static __device__ __forceinline__ Acc dbl_slow(const Acc& a) { return acc29::dbl_slow(a); }
  static __device__ __forceinline__ Raw raw_of(const Acc& a, bool zero) { return acc29::raw_of(a, zero); }
  static __device__ __forceinline__ XYZZ<Fq> to_xyzz(const Acc& a) { return acc29::to_xyzz(a); }
};
struct Pol28 {
  using Fq = Bls381Fq;
  using F = f28::F28;
  using Acc = acc28_core::Acc;
  // Raw: the accumulator as it is (14 x 28-bit limbs per coordinate, 224 B);
  // the identity is zz = 0 alone, as acc29::Raw
  using Raw = Acc;
  static __device__ __forceinline__ F shift_repack(const uint32_t* w) { return f28::shl8_repack(w); }
  // 257p with the low limbs raised by 2^28 (limbs < 2^29): 257p - y~ << 8 is a
  // borrow-free negation of the shifted canonical y~ (< 256p), < 257p -- inside
  // acc28's base bound of 512p (tests/test_f28_host.py)
  static constexpr uint32_t kK257[14] = {0x1faa55abu, 0x1feffffeu, 0x13ffb9b7u, 0x1feb0054u, 0x1a42caaau,
                                         0x197a7a70u, 0x16980372u, 0x17897d21u, 0x1bc2d077u, 0x1f8843bcu,
                                         0x135df98du, 0x180e566bu, 0x1c23b965u, 0x01a1b12eu};
  static __device__ __forceinline__ F repack_y(const Fq& y, uint32_t neg) {
    F r = f28::shl8_repack(y.v);
    const F m = f28::ksub(kK257, r);
#pragma unroll
    for (int i = 0; i < 14; ++i) r.l[i] = neg ? m.l[i] : r.l[i];
    return r;
  }
  static __device__ __forceinline__ Acc from_shifted(const F& x, const F& y) { return acc28_core::from_shifted(x, y); }
  static __device__ __forceinline__ Acc madd(const Acc& a, const F& x, const F& y, int* sp) {
    return acc28_core::madd(a, x, y, sp);
  }
  static __device__ __forceinline__ Acc dbl_slow(const Acc& a) { return acc28_core::dbl(a); }
  static __device__ __forceinline__ Raw raw_of(const Acc& a, bool zero) {
    Raw r = a;
#pragma unroll
    for (int k = 0; k < 14; ++k) r.zz.l[k] = zero ? 0u : a.zz.l[k];
    return r;
  }
  static __device__ __forceinline__ XYZZ<Fq> to_xyzz(const Acc& a) {
    XYZZ<Fq> r;
    f28::to32(a.x, r.x.v);
    f28::to32(a.y, r.y.v);
    f28::to32(a.zz, r.zz.v);
    f28::to32(a.zzz, r.zzz.v);
    return r;
  }
};

// kPrefetch: 0 = gather each base at its own iteration; 1 = the next base in
// registers (16 VGPRs: 186, two waves per SIMD); 2 = the next base through
// LDS by LDS-DMA (global_load_lds_dwordx4: no VGPR destination, so the
// kernel keeps its 3-wave register budget with the gather one iteration ahead)
typedef __attribute__((address_space(3))) void lds_void_t;
#ifndef TACHYON_GATHER_NT
#define TACHYON_GATHER_NT 0  // 1: nontemporal base gathers (A/B build)
#endif
// kEnt: how a lane reads its K sorted entries.  A lane's entries sit K x 8
// bytes from its neighbours', so a wave's entry load touches 64 lines, and
// the bases' gathers (~3.5 TB/s of lines) evict them from the XCD's L2
// before the lane's next iteration: an 8-byte load per iteration fetched a
// line per entry (123 vs 72 algorithmic HBM bytes per entry, FETCH_SIZE).
//   0: one 8-byte load per iteration, two ahead (rounds 1-6a)
//   1: aligned 16-byte pairs (entries 2m, 2m + 1), the next pair an iteration
//      ahead -- a line per two entries (FETCH 93.7 B per entry; 2^26
//      accumulation 59.6 -> 58.9 ms, profiles/r06h/ab_ent_pairs.log)
//   2: 64-byte chunks (8 entries) through LDS by LDS-DMA, the next chunk
//      8 iterations ahead, double-buffered: 8 KiB of LDS per wave (4 KiB per
//      buffer), 32 KiB per 256-thread workgroup, no VGPRs; the
//      lane's first entry must be 16-byte aligned (g0 even: gbeg and K even)
//      and the entry array 64 bytes longer than gend (MsmGpu::carve's
//      slack).  FETCH 72.4 B per entry = the 64-byte base + 8; 2^26
//      accumulation 58.8 -> 57.0 ms, BLS12-381 G1 2^24 31.4 -> 30.8 ms
//      (profiles/r06i/ab_entries_staged.log).  The default where g0 is even.
template <class Pol, int kPrefetch, bool kRaw, int kEnt = 0>
__device__ __forceinline__ void seg_acc_limb_body(const Affine<typename Pol::Fq>* __restrict__ bases,
                                                  const uint64_t* __restrict__ ents, uint32_t c, uint64_t gbeg,
                                                  uint64_t gend, uint64_t tbase, uint32_t K, uint32_t idx_mask,
                                                  XYZZ<typename Pol::Fq>* __restrict__ bucket_sum,
                                                  XYZZ<typename Pol::Fq>* __restrict__ pieces,
                                                  uint32_t* __restrict__ tflags, uint32_t* __restrict__ tlast) {
  static_assert(kEnt != 2 || kPrefetch == 0, "LDS-staged entries only with the unprefetched base gather");
  using Fq = typename Pol::Fq;
  using F = typename Pol::F;
  using Acc = typename Pol::Acc;
  const uint64_t tl = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t g0 = gbeg + tl * K;
  if (g0 >= gend) return;
  const uint64_t g1 = min(g0 + K, gend);
  const uint64_t t = tbase + tl;
  const uint32_t prev_b = g0 > gbeg ? bucket_of_key(entry_key(ents[g0 - 1]), c) : kNoBucket;
  const uint32_t next_b = (g1 < gend) ? bucket_of_key(entry_key(ents[g1]), c) : kNoBucket;
  uint32_t flags = 0, runs = 0, cur = kNoBucket;
  Acc acc{};  // (any defined value: the stores mask it while acc_zero)
  bool acc_zero = true;
  // kRaw: the accumulator as it is (Raw); otherwise R form, the identity as
  // zz = zzz = 0 (x, y are not read)
  auto put = [&](XYZZ<Fq>* dst, size_t i) {
    if constexpr (kRaw) {
      reinterpret_cast<typename Pol::Raw*>(dst)[i] = Pol::raw_of(acc, acc_zero);
    } else {
      XYZZ<Fq> s = Pol::to_xyzz(acc);
      const uint32_t keep = acc_zero ? 0u : ~0u;
#pragma unroll
      for (int k = 0; k < Fq::N; ++k) {
        s.zz.v[k] &= keep;
        s.zzz.v[k] &= keep;
      }
      dst[i] = s;
    }
  };
  uint64_t e0 = 0, e1 = 0;
  uint64_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;  // kEnt 1: entries 2m .. 2m + 3, m = g / 2
  auto load_pair = [&](uint64_t i, uint64_t& a, uint64_t& b) {  // entries i, i + 1 (i even), zeros past gend
    if (i + 1 < gend) {
      const uint4 v = *reinterpret_cast<const uint4*>(ents + i);
      a = (uint64_t)v.y << 32 | v.x;
      b = (uint64_t)v.w << 32 | v.z;
    } else {
      a = i < gend ? ents[i] : 0;
      b = 0;
    }
  };
  // kEnt 2: [buffer][wave][16-byte piece][lane]; chunk j of a lane (entries
  // g0 + 8j ..) in buffer j & 1
  __shared__ uint4 estage[kEnt == 2 ? 2 : 1][kEnt == 2 ? kBlock / 64 : 1][4][kEnt == 2 ? 64 : 1];
  const uint32_t ewave = threadIdx.x >> 6, elane = threadIdx.x & 63;
  auto fetch_chunk = [&](uint64_t first, uint32_t buf) {
    const uint4* src = reinterpret_cast<const uint4*>(ents + first);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_global_load_lds(src + q, (lds_void_t*)&estage[buf][ewave][q][0], 16, 0, 0);
  };
  if constexpr (kEnt == 1) {
    load_pair(g0 & ~uint64_t(1), q0, q1);
    load_pair((g0 & ~uint64_t(1)) + 2, q2, q3);
    e0 = (g0 & 1) ? q1 : q0;
    e1 = (g0 & 1) ? q2 : q1;
  } else if constexpr (kEnt == 2) {
    fetch_chunk(g0, 0);
  } else {
    e0 = ents[g0];
    e1 = (g0 + 1 < g1) ? ents[g0 + 1] : 0;
  }
  Affine<Fq> P;
  // LDS-DMA staging: [slot][wave][16-byte chunk][lane], 32 KiB per workgroup; a
  // wave-instruction writes its 64 lanes' chunks contiguously (base + 16 lane)
  __shared__ uint4 stage[kPrefetch == 2 ? 2 : 1][kPrefetch == 2 ? kBlock / 64 : 1][4][64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  auto issue = [&](uint64_t e, uint32_t slot) {  // the base of entry e into stage[slot]
    const uint4* src = reinterpret_cast<const uint4*>(bases + (entry_val(e) & idx_mask));
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      __builtin_amdgcn_global_load_lds(src + ch, (lds_void_t*)&stage[slot][wave][ch][0], 16, 0, TACHYON_GATHER_NT ? 2 : 0);
  };
  if constexpr (kPrefetch == 1) P = bases[entry_val(e0) & idx_mask];
  if constexpr (kPrefetch == 2) issue(e0, 0);
  uint32_t it = 0;  // iteration count: the same for every lane of the wave (K entries each)
  for (uint64_t g = g0; g < g1; ++g, ++it) {
    uint64_t e2 = 0;
    if constexpr (kEnt == 1) {
      // (g & 1 is the same for every lane of the wave when K and gbeg are even)
      if (g & 1) {  // entry g + 2 opens the next pair: shift, and load the one after
        e2 = q3;
        q0 = q2;
        q1 = q3;
        load_pair(g + 3, q2, q3);
      } else {
        e2 = q2;
      }
    } else if constexpr (kEnt == 2) {
      if ((it & 7) == 0) {  // a new chunk: it has landed (this wave's own LDS-DMA); fetch the next one
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (g + 8 < g1) fetch_chunk(g + 8, ((it >> 3) + 1) & 1);
      }
      const uint32_t sl = it & 7;
      const uint2 w = reinterpret_cast<const uint2*>(&estage[(it >> 3) & 1][ewave][sl >> 1][elane])[sl & 1];
      e0 = (uint64_t)w.y << 32 | w.x;
    } else {
      e2 = (g + 2 < g1) ? ents[g + 2] : 0;
    }
    Affine<Fq> Pn;
    if constexpr (kPrefetch == 1) {
      Pn = bases[entry_val(e1) & idx_mask];
    } else if constexpr (kPrefetch == 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this iteration's base has landed
      const uint32_t slot = it & 1;
      uint4 ch[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) ch[q] = stage[slot][wave][q][lane];
      memcpy(&P, ch, sizeof(P));
      if (g + 1 < g1) issue(e1, slot ^ 1);  // the next base, under this iteration's madd
    } else if constexpr (TACHYON_GATHER_NT) {  // A/B: the base gather with the nontemporal policy
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4* src = reinterpret_cast<const u32x4*>(bases + (entry_val(e0) & idx_mask));
      constexpr int kChunks = sizeof(Affine<Fq>) / 16;
      u32x4 ch[kChunks];
#pragma unroll
      for (int q = 0; q < kChunks; ++q) ch[q] = __builtin_nontemporal_load(src + q);
      memcpy(&P, ch, sizeof(P));
    } else {
      P = bases[entry_val(e0) & idx_mask];
    }
    const uint32_t k0 = entry_key(e0), v0 = entry_val(e0);
    const uint32_t b = bucket_of_key(k0, c);
    if (b != kNoBucket) {
      if (b != cur) {
        if (cur != kNoBucket) {
          // one store for both destinations (a head piece or the bucket's
          // sum): a single conversion block when the wave's lanes differ
          const bool head = runs == 1 && cur == prev_b;
          if (head) flags |= kHead;
          put(head ? pieces : bucket_sum, head ? 2 * t : cur);
        }
        cur = b;
        ++runs;
        acc_zero = true;
      }
      if (!P.is_zero_canonical()) {
        const F x2 = Pol::shift_repack(P.x.v), y2 = Pol::repack_y(P.y, v0 & kSignBit);  // both paths
        if (acc_zero) {
          acc = Pol::from_shifted(x2, y2);
          acc_zero = false;
        } else {
          int special = 0;
          acc = Pol::madd(acc, x2, y2, &special);  // (unchanged when special)
          if (special == 1) acc_zero = true;
          else if (special == 2) acc = Pol::dbl_slow(acc);
        }
      }
    }
    e0 = e1;
    e1 = e2;
    if constexpr (kPrefetch == 1) P = Pn;
  }
  if (cur != kNoBucket) {
    const bool head = runs == 1 && cur == prev_b;
    const bool tail = cur == next_b;
    if (head) { put(pieces, 2 * t); flags |= kHead; }
    if (tail) flags |= kTail;
    if (tail && !head) put(pieces, 2 * t + 1);
    if (!head && !tail) put(bucket_sum, cur);
  }
  if (runs <= 1) flags |= kSingle;
  acc_zero = true;  // absent pieces are the identity
  if (!(flags & kHead)) put(pieces, 2 * t);
  const bool through = (flags & kHead) && (flags & kTail) && (flags & kSingle);
  if (!(flags & kTail) || through) put(pieces, 2 * t + 1);
  tflags[t] = flags;
  tlast[t] = cur;
}


// (4 waves per SIMD -- <= 128 VGPRs, 14 spilled -- measured slower at 2^26:
// 76.1-76.4 vs 75.0-75.5 ms, profiles/r04b/tune_sort_tiles_recode_spt_4waves_2_24_26.log)
template <int kPrefetch, bool kRaw, int kEnt>
__global__ __launch_bounds__(kBlock, kPrefetch == 1 ? 1 : 3) void seg_acc29_kernel(const Affine<Bn254Fq>* __restrict__ bases,
                                                           const uint64_t* __restrict__ ents, uint32_t c,
                                                           uint64_t gbeg, uint64_t gend, uint64_t tbase, uint32_t K,
                                                           uint32_t idx_mask, XYZZ<Bn254Fq>* __restrict__ bucket_sum,
                                                           XYZZ<Bn254Fq>* __restrict__ pieces,
                                                           uint32_t* __restrict__ tflags, uint32_t* __restrict__ tlast) {
  seg_acc_limb_body<Pol29, kPrefetch, kRaw, kEnt>(bases, ents, c, gbeg, gend, tbase, K, idx_mask, bucket_sum, pieces,
                                                  tflags, tlast);
}
// BLS12-381 G1 over the 14 x 28-bit field: R-form stores (the FIPS chain join
// and window reductions read them); 2 waves per SIMD (the 14-limb madd holds
// ~4 x 14 accumulator + 2 x 14 base words)
template <int kEnt, bool kRaw>
__global__ __launch_bounds__(kBlock, 2) void seg_acc28_kernel(const Affine<Bls381Fq>* __restrict__ bases,
                                                              const uint64_t* __restrict__ ents, uint32_t c,
                                                              uint64_t gbeg, uint64_t gend, uint64_t tbase, uint32_t K,
                                                              uint32_t idx_mask,
                                                              XYZZ<Bls381Fq>* __restrict__ bucket_sum,
                                                              XYZZ<Bls381Fq>* __restrict__ pieces,
                                                              uint32_t* __restrict__ tflags,
                                                              uint32_t* __restrict__ tlast) {
  seg_acc_limb_body<Pol28, 0, kRaw, kEnt>(bases, ents, c, gbeg, gend, tbase, K, idx_mask, bucket_sum, pieces, tflags,
                                          tlast);
}

// ---------------------------------------------------------------------------
// G2 (Fq2) accumulation with a lane pair per virtual thread (acc_pair.h): the
// run logic of seg_acc_kernel, lane h holding component h of every Fq2 value.
// Both lanes of a pair read the same entries and take the same branches.
template <class Curve, bool kCall>
__global__ __launch_bounds__(kBlock) void seg_acc_pair_kernel(const Affine<typename Curve::F>* __restrict__ bases,
                                                              const uint64_t* __restrict__ ents, uint32_t c,
                                                              uint64_t gbeg, uint64_t gend, uint64_t tbase, uint32_t K,
                                                              uint32_t idx_mask,
                                                              XYZZ<typename Curve::F>* __restrict__ bucket_sum,
                                                              XYZZ<typename Curve::F>* __restrict__ pieces,
                                                              uint32_t* __restrict__ tflags,
                                                              uint32_t* __restrict__ tlast) {
  using Fb = typename Curve::F::Base;  // Fq
  using F = HotFp<Fb>;
  using namespace pair;
  using H = Half<F, kCall>;
  const uint32_t h = threadIdx.x & 1u;
  const uint64_t tl = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 1;
  const uint64_t g0 = gbeg + tl * K;
  if (g0 >= gend) return;  // both lanes of the pair
  const uint64_t g1 = min(g0 + K, gend);
  const uint64_t t = tbase + tl;
  const uint32_t prev_b = g0 > gbeg ? bucket_of_key(entry_key(ents[g0 - 1]), c) : kNoBucket;
  const uint32_t next_b = (g1 < gend) ? bucket_of_key(entry_key(ents[g1]), c) : kNoBucket;
  // component views: a point is {x.c0, x.c1, y.c0, y.c1}, an XYZZ {x.c0, x.c1, ..., zzz.c1}
  const Fb* comp = reinterpret_cast<const Fb*>(bases);
  Fb* bsum = reinterpret_cast<Fb*>(bucket_sum);
  Fb* pcs = reinterpret_cast<Fb*>(pieces);
  const F one_h = h ? F::zero() : F::one();
  Acc<H> acc;
  bool acc_zero = true;
  auto store = [&](Fb* dst, uint64_t idx) {  // this lane's components of the run sum (identity if none)
    Fb* o = dst + 8 * idx;
    if (acc_zero) {
      o[h] = one_h;
      o[2 + h] = one_h;
      o[4 + h] = Fb::zero();
      o[6 + h] = Fb::zero();
    } else {
      o[h] = acc.x.v;
      o[2 + h] = acc.y.v;
      o[4 + h] = acc.zz.v;
      o[6 + h] = acc.zzz.v;
    }
  };
  uint32_t flags = 0, runs = 0, cur = kNoBucket;
  uint64_t e0 = ents[g0];
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t e1 = (g + 1 < g1) ? ents[g + 1] : 0;
    const uint32_t k0 = entry_key(e0), v0 = entry_val(e0);
    const uint32_t b = bucket_of_key(k0, c);
    if (b != kNoBucket) {
      const Fb* pt = comp + 4 * (size_t)(v0 & idx_mask);
      H px{pt[h]}, py{pt[2 + h]};
      if (b != cur) {
        if (cur != kNoBucket) {
          if (runs == 1 && cur == prev_b) { store(pcs, 2 * t); flags |= kHead; }
          else store(bsum, cur);
        }
        cur = b;
        ++runs;
        acc_zero = true;
      }
      const uint32_t pz = (px.v.is_zero_canonical() && py.v.is_zero_canonical()) ? 1u : 0u;
      if (!(pz & dpp<kSwap>(pz))) {  // not the identity base (both components zero)
        py.v = py.v.cond_neg_canonical(v0 & kSignBit);
        if (acc_zero) {
          acc = Acc<H>{px, py, H{one_h}, H{one_h}};
          acc_zero = false;
        } else {
          int special = 0;
          acc = madd(acc, px, py, h != 0, &special);  // (unchanged when special)
          if (special == 1) acc_zero = true;
          else if (special == 2) acc = pair::dbl(acc, h != 0);
        }
      }
    }
    e0 = e1;
  }
  if (cur != kNoBucket) {
    const bool head = runs == 1 && cur == prev_b;
    const bool tail = cur == next_b;
    if (head) { store(pcs, 2 * t); flags |= kHead; }
    if (tail) flags |= kTail;
    if (tail && !head) store(pcs, 2 * t + 1);
    if (!head && !tail) store(bsum, cur);
  }
  if (runs <= 1) flags |= kSingle;
  acc_zero = true;  // absent pieces are the identity
  if (!(flags & kHead)) store(pcs, 2 * t);
  const bool through = (flags & kHead) && (flags & kTail) && (flags & kSingle);
  if (!(flags & kTail) || through) store(pcs, 2 * t + 1);
  if (h == 0) {
    tflags[t] = flags;
    tlast[t] = cur;
  }
}

// The limb-field lane pairs of G2 (field policies of seg_acc_pair_limb_kernel):
// BLS12-381 over the 14 x 28-bit Fq (msm/pair28.h), BN254 over the 9 x 29-bit
// Fq (msm/pair29.h).
struct PairPol28 {
  using Fb = Bls381Fq;
  using F2 = Bls381Fq2;
  using F = f28::F28;
  using Acc = pair28::Acc;
  static __device__ __forceinline__ F repack(const uint32_t* w) { return f28::shl8_repack(w); }
  static __device__ __forceinline__ Acc start(const F& x, const F& y, bool h) { return pair28::from_shifted(x, y, h); }
  static __device__ __forceinline__ Acc madd(const Acc& a, const F& x, const F& y, bool h, int* sp) {
    return pair28::madd(a, x, y, h, sp);
  }
  static __device__ __forceinline__ Acc dbl(const Acc& a, bool h) { return pair28::dbl(a, h); }
  static __device__ __forceinline__ Acc add(const Acc& a, const Acc& b, bool h, int* sp) {
    return pair28::add(a, b, h, sp);
  }
  static __device__ __forceinline__ void to32(const F& x, uint32_t* w) { f28::to32(x, w); }
  static __device__ __forceinline__ F from32(const uint32_t* w) { return f28::from32(w); }
};
struct PairPol29 {
  using Fb = Bn254Fq;
  using F2 = Bn254Fq2;
  using F = f29::F29;
  using Acc = pair29::Acc;
  static __device__ __forceinline__ F repack(const uint32_t* w) { return f29::shl5_repack(w); }
  static __device__ __forceinline__ Acc start(const F& x, const F& y, bool h) { return pair29::from_shifted(x, y, h); }
  static __device__ __forceinline__ Acc madd(const Acc& a, const F& x, const F& y, bool h, int* sp) {
    return pair29::madd(a, x, y, h, sp);
  }
  static __device__ __forceinline__ Acc dbl(const Acc& a, bool h) { return pair29::dbl(a, h); }
  static __device__ __forceinline__ Acc add(const Acc& a, const Acc& b, bool h, int* sp) {
    return pair29::add(a, b, h, sp);
  }
  static __device__ __forceinline__ void to32(const F& x, uint32_t* w) { f29::to32(x, w); }
  static __device__ __forceinline__ F from32(const uint32_t* w) { return f29::from32(w); }
};

// G2 with a lane pair per point over a limb field: seg_acc_pair_kernel's run
// logic; the stores convert this lane's components to the R form the
// lane-pair FIPS reductions read.  set_variant bit 20 restores the FIPS pair.
// kStaged: the entries in 64-byte chunks through LDS as seg_acc_limb_body's
// kEnt 2 (a pair's two lanes DMA the chunk's four 16-byte pieces, two each;
// g0 even and 64 bytes of slack after the entry array)
template <class Pol, bool kStaged, bool kRaw>
__global__ __launch_bounds__(kBlock) void seg_acc_pair_limb_kernel(const Affine<typename Pol::F2>* __restrict__ bases,
                                                                   const uint64_t* __restrict__ ents, uint32_t c,
                                                                   uint64_t gbeg, uint64_t gend, uint64_t tbase,
                                                                   uint32_t K, uint32_t idx_mask,
                                                                   XYZZ<typename Pol::F2>* __restrict__ bucket_sum,
                                                                   XYZZ<typename Pol::F2>* __restrict__ pieces,
                                                                   uint32_t* __restrict__ tflags,
                                                                   uint32_t* __restrict__ tlast) {
  using Fb = typename Pol::Fb;
  using F = typename Pol::F;
  using Acc = typename Pol::Acc;
  const uint32_t h = threadIdx.x & 1u;
  const uint64_t tl = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 1;
  const uint64_t g0 = gbeg + tl * K;
  if (g0 >= gend) return;  // both lanes of the pair
  const uint64_t g1 = min(g0 + K, gend);
  const uint64_t t = tbase + tl;
  const uint32_t prev_b = g0 > gbeg ? bucket_of_key(entry_key(ents[g0 - 1]), c) : kNoBucket;
  const uint32_t next_b = (g1 < gend) ? bucket_of_key(entry_key(ents[g1]), c) : kNoBucket;
  const Fb* comp = reinterpret_cast<const Fb*>(bases);
  Fb* bsum = reinterpret_cast<Fb*>(bucket_sum);
  Fb* pcs = reinterpret_cast<Fb*>(pieces);
  const Fb one_h = h ? Fb::zero() : Fb::one();
  Acc acc{};  // (any defined value: the raw stores mask it while acc_zero)
  bool acc_zero = true;
  auto store = [&](Fb* dst, uint64_t idx) {  // this lane's components of the run sum (identity if none)
    if constexpr (kRaw) {  // the limbs as they are (LimbPairArith<Pol, true>::load), identity = zz zero
      F* o = reinterpret_cast<F*>(dst) + 8 * idx;
      F zz = acc.zz;
#pragma unroll
      for (int k = 0; k < (int)(sizeof(F) / 4); ++k) zz.l[k] = acc_zero ? 0u : zz.l[k];
      o[h] = acc.x;
      o[2 + h] = acc.y;
      o[4 + h] = zz;
      o[6 + h] = acc.zzz;
      return;
    }
    Fb* o = dst + 8 * idx;
    if (acc_zero) {
      o[h] = one_h;
      o[2 + h] = one_h;
      o[4 + h] = Fb::zero();
      o[6 + h] = Fb::zero();
    } else {
      Fb v;
      Pol::to32(acc.x, v.v);
      o[h] = v;
      Pol::to32(acc.y, v.v);
      o[2 + h] = v;
      Pol::to32(acc.zz, v.v);
      o[4 + h] = v;
      Pol::to32(acc.zzz, v.v);
      o[6 + h] = v;
    }
  };
  uint32_t flags = 0, runs = 0, cur = kNoBucket;
  // [buffer][wave][piece pair q][lane]: lane 2 vt + h' holds piece 2q + h' of virtual thread vt's chunk
  __shared__ uint4 estage[kStaged ? 2 : 1][kStaged ? kBlock / 64 : 1][2][kStaged ? 64 : 1];
  const uint32_t ewave = threadIdx.x >> 6, elane = threadIdx.x & 63;
  auto fetch_chunk = [&](uint64_t first, uint32_t buf) {
    const uint4* src = reinterpret_cast<const uint4*>(ents + first) + h;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_global_load_lds(src + 2 * q, (lds_void_t*)&estage[buf][ewave][q][0], 16, 0, 0);
  };
  uint64_t e0 = 0;
  if constexpr (kStaged) fetch_chunk(g0, 0);
  else e0 = ents[g0];
  uint32_t it = 0;  // (the same for both lanes of a pair and every pair of the wave)
  for (uint64_t g = g0; g < g1; ++g, ++it) {
    uint64_t e1 = 0;
    if constexpr (kStaged) {
      if ((it & 7) == 0) {  // a new chunk: landed (this wave's own LDS-DMA); fetch the next one
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (g + 8 < g1) fetch_chunk(g + 8, ((it >> 3) + 1) & 1);
      }
      const uint32_t sl = it & 7, piece = sl >> 1;
      const uint2 w = reinterpret_cast<const uint2*>(
          &estage[(it >> 3) & 1][ewave][piece >> 1][(elane & ~1u) | (piece & 1)])[sl & 1];
      e0 = (uint64_t)w.y << 32 | w.x;
    } else {
      e1 = (g + 1 < g1) ? ents[g + 1] : 0;
    }
    const uint32_t k0 = entry_key(e0), v0 = entry_val(e0);
    const uint32_t b = bucket_of_key(k0, c);
    if (b != kNoBucket) {
      const Fb* pt = comp + 4 * (size_t)(v0 & idx_mask);
      const Fb px = pt[h];
      Fb py = pt[2 + h];
      if (b != cur) {
        if (cur != kNoBucket) {  // (one store block for both destinations, as seg_acc_limb_body)
          const bool head = runs == 1 && cur == prev_b;
          if (head) flags |= kHead;
          store(head ? pcs : bsum, head ? 2 * t : cur);
        }
        cur = b;
        ++runs;
        acc_zero = true;
      }
      const uint32_t pz = (px.is_zero_canonical() && py.is_zero_canonical()) ? 1u : 0u;
      if (!(pz & pair::dpp<pair::kSwap>(pz))) {  // not the identity base (both components zero)
        py = py.cond_neg_canonical(v0 & kSignBit);
        const F x2 = Pol::repack(px.v), y2 = Pol::repack(py.v);
        if (acc_zero) {
          acc = Pol::start(x2, y2, h != 0);
          acc_zero = false;
        } else {
          int special = 0;
          acc = Pol::madd(acc, x2, y2, h != 0, &special);  // (unchanged when special)
          if (special == 1) acc_zero = true;
          else if (special == 2) acc = Pol::dbl(acc, h != 0);
        }
      }
    }
    if constexpr (!kStaged) e0 = e1;
  }
  if (cur != kNoBucket) {
    const bool head = runs == 1 && cur == prev_b;
    const bool tail = cur == next_b;
    if (head) { store(pcs, 2 * t); flags |= kHead; }
    if (tail) flags |= kTail;
    if (tail && !head) store(pcs, 2 * t + 1);
    if (!head && !tail) store(bsum, cur);
  }
  if (runs <= 1) flags |= kSingle;
  acc_zero = true;  // absent pieces are the identity
  if (!(flags & kHead)) store(pcs, 2 * t);
  const bool through = (flags & kHead) && (flags & kTail) && (flags & kSingle);
  if (!(flags & kTail) || through) store(pcs, 2 * t + 1);
  if (h == 0) {
    tflags[t] = flags;
    tlast[t] = cur;
  }
}

}  // namespace
}  // namespace detail
}  // namespace tachyon_amd::msm
