// MSM stage 4, chain join: the chain tables, the join levels' offsets, the reduction
// arithmetic policies and the seg_reduce kernels (part of msm_impl.h).
#pragma once

namespace tachyon_amd::msm {
namespace detail {
namespace {  // internal linkage: every per-curve TU gets its own copy

// A bucket that crosses thread boundaries forms a chain t0 < ... < t1: the
// tail of t0, the whole-range heads of the "through" threads in between and
// the head of t1 -- i.e. pieces[2*t0+1 .. 2*t1] (absent tails are identity).
__device__ __forceinline__ bool chain_start(uint32_t f) {
  const bool through = (f & kHead) && (f & kTail) && (f & kSingle);
  return (f & kTail) && !through;
}
__device__ __forceinline__ bool chain_end(uint32_t f) {
  const bool through = (f & kHead) && (f & kTail) && (f & kSingle);
  return (f & kHead) && !through;
}

// The accumulation's run flags (kHead / kTail / kSingle) and last bucket of
// every thread, from the sorted keys alone: the values seg_acc*_kernel writes
// (head = the first run continues the previous thread's last bucket, tail =
// the last run continues into the next thread, single = at most one run).  So
// the chain tables below can be built on a second stream WHILE the
// accumulation runs, and the host's read-back of the chain count and length
// hides behind it (small MSMs: the tables, the read-back and the join-level
// offsets were ~90 us on the critical path of a 0.7 ms 2^16 MSM).  Keys are
// sorted, so equal first and last buckets mean one run; the loop runs only
// when an end of the range holds digit-0 entries (no bucket).
// Debug check (set_variant bit 21): the run flags chain_flags_kernel derived
// from the sorted keys before the accumulation equal the ones the accumulation
// wrote (the small-MSM chain tables are built from the former).
__global__ __launch_bounds__(kBlock) void chain_flags_check_kernel(const uint32_t* __restrict__ tflags,
                                                                   const uint32_t* __restrict__ tlast,
                                                                   const uint32_t* __restrict__ cflags,
                                                                   const uint32_t* __restrict__ clast, uint32_t T,
                                                                   uint32_t* __restrict__ mismatches) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= T) return;
  if (tflags[t] != cflags[t] || tlast[t] != clast[t]) atomicAdd(mismatches, 1u);
}

__global__ __launch_bounds__(kBlock) void chain_flags_kernel(const uint64_t* __restrict__ ents, uint32_t c,
                                                             uint64_t gbeg, uint64_t gend, uint32_t K, uint32_t T,
                                                             uint32_t* __restrict__ tflags,
                                                             uint32_t* __restrict__ tlast) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= T) return;
  const uint64_t g0 = gbeg + (uint64_t)t * K, g1 = min(g0 + K, gend);
  auto bucket = [&](uint64_t g) -> uint32_t { return bucket_of_key(entry_key(ents[g]), c); };
  const uint32_t prev_b = g0 > gbeg ? bucket(g0 - 1) : kNoBucket;
  const uint32_t next_b = g1 < gend ? bucket(g1) : kNoBucket;
  uint32_t first = bucket(g0), last = bucket(g1 - 1);
  bool single = first == last;
  if (first == kNoBucket || last == kNoBucket) {
    uint32_t runs = 0, cur = kNoBucket;
    first = kNoBucket;
    for (uint64_t g = g0; g < g1; ++g) {
      const uint32_t b = bucket(g);
      if (b != kNoBucket && b != cur) {
        if (runs == 0) first = b;
        cur = b;
        ++runs;
      }
    }
    last = cur;
    single = runs <= 1;
  }
  uint32_t flags = single ? kSingle : 0u;
  if (first != kNoBucket && first == prev_b) flags |= kHead;
  if (last != kNoBucket && last == next_b) flags |= kTail;
  tflags[t] = flags;
  tlast[t] = last;
}

__global__ __launch_bounds__(kBlock) void chain_mark_kernel(const uint32_t* __restrict__ tflags, uint32_t T,
                                                            uint32_t* __restrict__ is_start,
                                                            uint32_t* __restrict__ max_len) {
  uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t == 0) *max_len = 0;  // seg_count_kernel's atomicMax target (no memset launch)
  if (t > T) return;
  is_start[t] = (t < T && chain_start(tflags[t])) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void chain_build_kernel(const uint32_t* __restrict__ tflags,
                                                             const uint32_t* __restrict__ tlast,
                                                             const uint32_t* __restrict__ cid, uint32_t T,
                                                             uint32_t* __restrict__ cbeg, uint32_t* __restrict__ cend,
                                                             uint32_t* __restrict__ cbucket,
                                                             uint32_t* __restrict__ nchains) {
  uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= T) return;
  uint32_t f = tflags[t];
  if (chain_end(f)) cend[cid[t] - 1] = 2 * t + 1;  // the chain opened by the last start before t
  if (chain_start(f)) {
    cbeg[cid[t]] = 2 * t + 1;
    cbucket[cid[t]] = tlast[t];
  }
  if (t == T - 1) nchains[0] = cid[t] + (chain_start(f) ? 1u : 0u);
}

// per-chain piece count for the first reduction level, and the longest chain
__global__ __launch_bounds__(kBlock) void seg_count_kernel(const uint32_t* __restrict__ beg,
                                                           const uint32_t* __restrict__ end,
                                                           const uint32_t* __restrict__ nseg_ptr, uint32_t nseg_cap,
                                                           unsigned K2, uint32_t* __restrict__ cnt,
                                                           uint32_t* __restrict__ max_len) {
  uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t nseg = nseg_ptr ? *nseg_ptr : nseg_cap;
  uint32_t len = 0;
  if (s < nseg) {
    len = end[s] - beg[s];
    cnt[s] = (len + K2 - 1) / K2;
  } else if (s <= nseg_cap) {
    cnt[s] = 0;
  }
  if (max_len) {
    __shared__ uint32_t red[kBlock / 64];
    for (int o = 32; o > 0; o >>= 1) len = max(len, (uint32_t)__shfl_xor(len, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t m = red[0];
      for (unsigned i = 1; i < kBlock / 64; ++i) m = max(m, red[i]);
      if (m) atomicMax(max_len, m);
    }
  }
}

// A join level's output offsets in ONE workgroup when there are few chains:
// off[s] = sum over s' < s of ceil(len_s' / K2), len_s = end[s] - beg[s]
// (end = nullptr: end[s] = beg[s + 1]).  Replaces seg_count + rocPRIM's
// two-kernel scan (three launches of a few microseconds on a latency-bound
// level) for nseg <= kJoinSmallChains.
constexpr unsigned kJoinOffBlock = 1024, kJoinSmallChains = 64 * 1024;
enum ChainMode { kChainsInStream, kChainsBefore, kChainsAfter };  // see MsmGpu::make_shape
__device__ __forceinline__ void join_offsets_body(const uint32_t* __restrict__ beg, const uint32_t* __restrict__ end,
                                                  uint32_t nseg, unsigned K2, uint32_t* __restrict__ off,
                                                  uint32_t* part) {
  const uint32_t t = threadIdx.x, per = (nseg + kJoinOffBlock - 1) / kJoinOffBlock;
  const uint32_t s0 = min(nseg, t * per), s1 = min(nseg, s0 + per);
  auto count = [&](uint32_t s) {
    const uint32_t len = (end ? end[s] : beg[s + 1]) - beg[s];
    return (len + K2 - 1) / K2;
  };
  uint32_t sum = 0;
  for (uint32_t s = s0; s < s1; ++s) sum += count(s);
  part[t] = sum;
  __syncthreads();
  for (unsigned d = 1; d < kJoinOffBlock; d <<= 1) {  // inclusive scan of the per-thread sums
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;  // exclusive prefix of this thread's range
  for (uint32_t s = s0; s < s1; ++s) {
    off[s] = run;
    run += count(s);
  }
  if (t == kJoinOffBlock - 1) off[nseg] = part[t];
}
__global__ __launch_bounds__(kJoinOffBlock) void join_offsets_kernel(const uint32_t* __restrict__ beg,
                                                                     const uint32_t* __restrict__ end, uint32_t nseg,
                                                                     unsigned K2, uint32_t* __restrict__ off) {
  __shared__ uint32_t part[kJoinOffBlock];
  join_offsets_body(beg, end, nseg, K2, off, part);
}

// The join levels' count and fan-in from the longest chain (the host makes
// the same choice from the read-back): 4-ary levels when a chain is longer
// than K2 pieces and the accumulation ran fewer than 2^20 threads
constexpr unsigned kJoinFanLong = 4;  // chain-join fan-in for chains longer than MsmPlan::K2
__host__ __device__ __forceinline__ unsigned join_fan_in(uint32_t max_len, unsigned K2, size_t T) {
  return (max_len > K2 && T < (size_t(1) << 20)) ? kJoinFanLong : K2;
}
__host__ __device__ __forceinline__ unsigned join_levels(uint32_t max_len, unsigned K2) {
  unsigned levels = 0;
  for (uint32_t len = max_len; len > 1; len = (len + K2 - 1) / K2) ++levels;
  return levels;
}

// Every join level's output offsets in one workgroup, BEFORE the
// accumulation (small MSMs): the chain count and the longest chain come from
// the chain tables in device memory (dscal), so nothing waits for the host;
// level l's table at ltab + l * stride (stride = T + 2 >= chains + 2).
__global__ __launch_bounds__(kJoinOffBlock) void join_offsets_all_kernel(const uint32_t* __restrict__ beg,
                                                                         const uint32_t* __restrict__ end,
                                                                         const uint32_t* __restrict__ dscal,
                                                                         unsigned K2base, uint32_t T, unsigned lv_max,
                                                                         size_t stride, uint32_t* __restrict__ ltab) {
  __shared__ uint32_t part[kJoinOffBlock];
  const uint32_t nseg = dscal[0], max_len = dscal[1];
  if (nseg == 0) return;
  const unsigned K2 = join_fan_in(max_len, K2base, T);
  const unsigned levels = min(join_levels(max_len, K2), lv_max);
  for (unsigned l = 0; l < levels; ++l) {
    const uint32_t* pbeg = l == 0 ? beg : ltab + (l - 1) * stride;
    join_offsets_body(pbeg, l == 0 ? end : nullptr, nseg, K2, ltab + l * stride, part);
    __syncthreads();  // the next level reads this table
  }
}

// largest s in [0, nseg) with off[s] <= t  (off non-decreasing)
__device__ __forceinline__ uint32_t find_segment(const uint32_t* __restrict__ off, uint32_t nseg, uint32_t t) {
  uint32_t lo = 0, hi = nseg;
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// The arithmetic of the one-lane reductions: the FIPS field (XYZZ<HotFp>, the
// arrays as they are) or a limb field (BLS12-381 G1 over 14 x 28-bit limbs,
// msm/acc28.h) that converts the R-form arrays on load (from32, < 3p) and
// store (to32), identities as flags.
template <class Curve>
struct FipsArith {
  using F = typename HotOf<typename Curve::F>::type;  // inline products (same layout)
  using A = XYZZ<F>;
  static __device__ __forceinline__ A load(const XYZZ<typename Curve::F>* p, size_t i) {
    return reinterpret_cast<const XYZZ<F>*>(p)[i];
  }
  static __device__ __forceinline__ void store(XYZZ<typename Curve::F>* p, size_t i, const A& a) {
    reinterpret_cast<XYZZ<F>*>(p)[i] = a;
  }
  static __device__ __forceinline__ A add(const A& a, const A& b) { return a + b; }
  static __device__ __forceinline__ A zero() { return A::zero(); }
  static __device__ __forceinline__ A dbl(const A& a) { return a.dbl(); }
  static __device__ __forceinline__ bool is_zero(const A& a) { return a.is_zero(); }
};
// kRawIn / kRawOut: the arrays hold Pol28::Raw (224-byte accumulator limbs,
// the identity as zz = 0) instead of R-form XYZZ -- the accumulation's raw
// stores read by the chain join and the window segments without conversions
// (madd's and add's outputs, X < 9.02p, Y, ZZ, ZZZ < 1.05p, are inside add's
// input invariant, msm/acc28.h)
template <bool kRawIn, bool kRawOut>
struct Limb28ArithT {
  using Fq = Bls381Fq;
  struct A {
    acc28_core::Acc a;
    bool zero;
  };
  static __device__ __forceinline__ A load(const XYZZ<Fq>* p, size_t i) {
    if constexpr (kRawIn) {
      const acc28_core::Acc r = reinterpret_cast<const acc28_core::Acc*>(p)[i];
      uint32_t nz = 0;
#pragma unroll
      for (int k = 0; k < 14; ++k) nz |= r.zz.l[k];
      return {r, nz == 0};
    } else {
      const XYZZ<Fq> q = p[i];
      if (q.is_zero()) return {acc28_core::Acc{}, true};
      return {{f28::from32(q.x.v), f28::from32(q.y.v), f28::from32(q.zz.v), f28::from32(q.zzz.v)}, false};
    }
  }
  static __device__ __forceinline__ void store(XYZZ<Fq>* p, size_t i, const A& a) {
    if constexpr (kRawOut) {
      reinterpret_cast<acc28_core::Acc*>(p)[i] = Pol28::raw_of(a.a, a.zero);
      return;
    }
    if (a.zero) {
      p[i] = XYZZ<Fq>::zero();
      return;
    }
    XYZZ<Fq> r;
    f28::to32(a.a.x, r.x.v);
    f28::to32(a.a.y, r.y.v);
    f28::to32(a.a.zz, r.zz.v);
    f28::to32(a.a.zzz, r.zzz.v);
    p[i] = r;
  }
  static __device__ __forceinline__ A add(const A& a, const A& b) {
    if (a.zero) return b;
    if (b.zero) return a;
    int special = 0;
    const acc28_core::Acc s = acc28_core::add(a.a, b.a, &special);
    if (special == 1) return {a.a, true};
    return {special == 2 ? acc28_core::dbl(a.a) : s, false};
  }
  static __device__ __forceinline__ A zero() { return {acc28_core::Acc{}, true}; }
  static __device__ __forceinline__ A dbl(const A& a) {  // (no point of this prime-order group doubles to the identity)
    return a.zero ? a : A{acc28_core::dbl(a.a), false};
  }
  static __device__ __forceinline__ bool is_zero(const A& a) { return a.zero; }
};
using Limb28Arith = Limb28ArithT<false, false>;

// One K2-ary level of the segmented tree: output q of segment s is the sum of
// in[beg[s] + q*K2 .. min(end[s], +K2)).  On the last level every segment has
// one output, which goes to bucket_sum[bucket[s]].
template <class Curve, class Ar = FipsArith<Curve>>
__global__ __launch_bounds__(kBlock, AccWaves<Curve>::value) void seg_reduce_kernel(const XYZZ<typename Curve::F>* __restrict__ in,
                                                            const uint32_t* __restrict__ beg,
                                                            const uint32_t* __restrict__ end,
                                                            const uint32_t* __restrict__ out_off, uint32_t nseg,
                                                            unsigned K2, XYZZ<typename Curve::F>* __restrict__ out,
                                                            const uint32_t* __restrict__ bucket,
                                                            XYZZ<typename Curve::F>* __restrict__ bucket_sum) {
  uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= out_off[nseg]) return;
  uint32_t s = find_segment(out_off, nseg, t);
  uint32_t q = t - out_off[s];
  uint32_t e0 = beg[s] + q * K2;
  uint32_t e1 = min(end[s], e0 + K2);
  typename Ar::A acc = Ar::load(in, e0);
  for (uint32_t e = e0 + 1; e < e1; ++e) acc = Ar::add(acc, Ar::load(in, e));
  if (bucket) Ar::store(bucket_sum, bucket[s], acc);
  else Ar::store(out, t, acc);
}

// The G2 reductions with a lane pair per point (acc_pair.h): the one-lane
// XYZZ<Fq2> additions hold two points and their temporaries (BLS12-381:
// 220-460 spilled VGPRs per kernel, 21 ms of a 2^24 MSM); split by component
// they stay in registers.  Same schedules as the one-lane kernels above.
// The arithmetic of the pair reductions: the FIPS lane pair (acc_pair.h) or a
// limb-field pair (msm/pair28.h, pair29.h) that converts the R-form arrays on
// load (from32, < 3p) and store (to32), keeping identities as flags.
template <class Curve>
struct FipsPairArith {
  using Fb = typename Curve::F::Base;
  using H = pair::Half<HotFp<Fb>, Fb::N == 12>;
  using A = pair::Acc<H>;
  static __device__ __forceinline__ A load(const Fb* p, size_t i, uint32_t h) { return pair::load<H>(p, i, h); }
  static __device__ __forceinline__ void store(Fb* p, size_t i, uint32_t h, const A& a) { pair::store(p, i, h, a); }
  static __device__ __forceinline__ A add(const A& a, const A& b, bool h) { return pair::add(a, b, h); }
  static __device__ __forceinline__ A zero(bool h) { return pair::zero<H>(h); }
  static __device__ __forceinline__ A small_mul(const A& P, uint32_t m, bool h) { return pair::small_mul(P, m, h); }
};
// kRawIn / kRawOut: the arrays hold the lane pair's limb-field components
// as they are (8 Pol::F per point: x, y, zz, zzz x 2 components; the identity
// = zz zero in both) instead of R-form Fq2 XYZZ: the raw accumulation stores,
// read by the chain join and the window segments (madd's and add's outputs
// keep add's input invariant X < 10p, Y < 6p, ZZ, ZZZ < 3p, msm/pair28.h,
// pair29.h)
template <class Pol, bool kRawIn = false, bool kRawOut = false>
struct LimbPairArith {
  using Fb = typename Pol::Fb;
  using F = typename Pol::F;
  struct A {
    typename Pol::Acc a;
    bool zero;
  };
  static __device__ __forceinline__ A load(const Fb* p, size_t i, uint32_t h) {
    if constexpr (kRawIn) {
      const F* o = reinterpret_cast<const F*>(p) + 8 * i;
      const F x = o[h], y = o[2 + h], zz = o[4 + h], zzz = o[6 + h];
      uint32_t nz = 0;
#pragma unroll
      for (int k = 0; k < (int)(sizeof(F) / 4); ++k) nz |= zz.l[k];
      nz |= pair::dpp<pair::kSwap>(nz);
      return {{x, y, zz, zzz}, nz == 0};
    }
    const Fb* o = p + 8 * i;
    const Fb x = o[h], y = o[2 + h], zz = o[4 + h], zzz = o[6 + h];
    uint32_t nz = 0;
#pragma unroll
    for (int k = 0; k < Fb::N; ++k) nz |= zz.v[k];
    nz |= pair::dpp<pair::kSwap>(nz);  // the identity: zz = 0 in both components
    return {{Pol::from32(x.v), Pol::from32(y.v), Pol::from32(zz.v), Pol::from32(zzz.v)}, nz == 0};
  }
  static __device__ __forceinline__ void store(Fb* p, size_t i, uint32_t h, const A& a) {
    if constexpr (kRawOut) {
      F* o = reinterpret_cast<F*>(p) + 8 * i;
      F zz = a.a.zz;
#pragma unroll
      for (int k = 0; k < (int)(sizeof(F) / 4); ++k) zz.l[k] = a.zero ? 0u : zz.l[k];
      o[h] = a.a.x;
      o[2 + h] = a.a.y;
      o[4 + h] = zz;
      o[6 + h] = a.a.zzz;
      return;
    }
    Fb* o = p + 8 * i;
    if (a.zero) {
      const Fb one_h = h ? Fb::zero() : Fb::one();
      o[h] = one_h;
      o[2 + h] = one_h;
      o[4 + h] = Fb::zero();
      o[6 + h] = Fb::zero();
      return;
    }
    Fb v;
    Pol::to32(a.a.x, v.v);
    o[h] = v;
    Pol::to32(a.a.y, v.v);
    o[2 + h] = v;
    Pol::to32(a.a.zz, v.v);
    o[4 + h] = v;
    Pol::to32(a.a.zzz, v.v);
    o[6 + h] = v;
  }
  static __device__ __forceinline__ A add(const A& a, const A& b, bool h) {
    if (a.zero) return b;
    if (b.zero) return a;
    int special = 0;
    const typename Pol::Acc s = Pol::add(a.a, b.a, h, &special);
    if (special == 1) return {a.a, true};
    return {special == 2 ? Pol::dbl(a.a, h) : s, false};
  }
  static __device__ __forceinline__ A zero(bool) { return {typename Pol::Acc{}, true}; }
  static __device__ __forceinline__ A small_mul(const A& P, uint32_t m, bool h) {
    if (m == 0 || P.zero) return zero(h);
    A r = P;
    for (int bit = 30 - __builtin_clz(m); bit >= 0; --bit) {
      r.a = Pol::dbl(r.a, h);  // (no point of this prime-order group doubles to the identity)
      if ((m >> bit) & 1) r = add(r, P, h);
    }
    return r;
  }
};

template <class Curve, class Ar = FipsPairArith<Curve>>
__global__ __launch_bounds__(kBlock, 2) void seg_reduce_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ in,
                                                                 const uint32_t* __restrict__ beg,
                                                                 const uint32_t* __restrict__ end,
                                                                 const uint32_t* __restrict__ out_off, uint32_t nseg,
                                                                 unsigned K2, XYZZ<typename Curve::F>* __restrict__ out,
                                                                 const uint32_t* __restrict__ bucket,
                                                                 XYZZ<typename Curve::F>* __restrict__ bucket_sum) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= out_off[nseg]) return;  // both lanes of the pair
  const uint32_t s = find_segment(out_off, nseg, t);
  const uint32_t e0 = beg[s] + (t - out_off[s]) * K2;
  const uint32_t e1 = min(end[s], e0 + K2);
  const Fb* src = reinterpret_cast<const Fb*>(in);
  typename Ar::A acc = Ar::load(src, e0, h);
  for (uint32_t e = e0 + 1; e < e1; ++e) acc = Ar::add(acc, Ar::load(src, e, h), h != 0);
  if (bucket) Ar::store(reinterpret_cast<Fb*>(bucket_sum), bucket[s], h, acc);
  else Ar::store(reinterpret_cast<Fb*>(out), t, h, acc);
}

// The BN254 G1 reductions over the 29-bit field (acc29::add / dbl; R-form
// arrays in and out, converted on load and store): the chain join and the
// window sums are chains of dependent point additions that run at one or two
// waves per SIMD, so an addition's instruction count is its latency.
template <bool kInRaw, bool kOutRaw>
__global__ __launch_bounds__(kBlock, 2) void seg_reduce29_kernel(const XYZZ<Bn254Fq>* __restrict__ in,
                                                                const uint32_t* __restrict__ beg,
                                                                const uint32_t* __restrict__ end,
                                                                const uint32_t* __restrict__ out_off, uint32_t nseg,
                                                                unsigned K2, XYZZ<Bn254Fq>* __restrict__ out,
                                                                const uint32_t* __restrict__ bucket,
                                                                XYZZ<Bn254Fq>* __restrict__ bucket_sum) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= out_off[nseg]) return;
  const uint32_t s = find_segment(out_off, nseg, t);
  const uint32_t e0 = beg[s] + (t - out_off[s]) * K2;
  const uint32_t e1 = min(end[s], e0 + K2);
  auto load = [&](uint32_t e) { return kInRaw ? acc29::load_raw(in, e) : acc29::load_pt(in, e); };
  acc29::Pt acc = load(e0);
  for (uint32_t e = e0 + 1; e < e1; ++e) acc = acc29::add(acc, load(e));
  if (bucket) {
    if constexpr (kOutRaw) acc29::store_raw(bucket_sum, bucket[s], acc);
    else acc29::store_pt(bucket_sum, bucket[s], acc);
  } else {
    acc29::store_pt(out, t, acc);
  }
}

}  // namespace
}  // namespace detail
}  // namespace tachyon_amd::msm
