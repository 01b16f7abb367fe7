// MSM stage 5, window sums: every window_* and reduce_uniform* kernel (part of msm_impl.h;
// the arithmetic policies are in msm_join.h).
#pragma once

namespace tachyon_amd::msm {
namespace detail {
namespace {  // internal linkage: every per-curve TU gets its own copy

// m * P for a small non-negative integer m (double-and-add, high bit first)
template <class F>
__device__ XYZZ<F> small_mul(const XYZZ<F>& P, uint32_t m) {
  XYZZ<F> r = XYZZ<F>::zero();
  if (m == 0 || P.is_zero()) return r;
  int top = 31 - __builtin_clz(m);
  r = P;
  for (int bit = top - 1; bit >= 0; --bit) {
    r = r.dbl();
    if ((m >> bit) & 1) r = r + P;
  }
  return r;
}
template <class Ar>
__device__ typename Ar::A small_mul_ar(const typename Ar::A& P, uint32_t m) {
  if (m == 0 || Ar::is_zero(P)) return Ar::zero();
  typename Ar::A r = P;
  for (int bit = 30 - __builtin_clz(m); bit >= 0; --bit) {
    r = Ar::dbl(r);
    if ((m >> bit) & 1) r = Ar::add(r, P);
  }
  return r;
}

// Window reduction, stage 1: segment j of window w covers buckets
// [j*L, (j+1)*L) (bucket b holds |digit| = b+1).  Running sums from the top
// give S = sum (b - jL + 1) B_b and R = sum B_b; the segment's share of
// sum_b (b+1) B_b is S + jL * R  (PippengerBase::AccumulateBuckets,
// pippenger_base.h:36-57, split across threads).
template <class Curve, class Ar = FipsArith<Curve>>
__global__ __launch_bounds__(kBlock, AccWaves<Curve>::value) void window_segment_kernel(const XYZZ<typename Curve::F>* __restrict__ bucket_sum,
                                                                unsigned W, unsigned B, unsigned L,
                                                                XYZZ<typename Curve::F>* __restrict__ out) {
  uint32_t S = B / L;
  uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= W * S) return;
  uint32_t w = t / S, j = t - w * S;
  const size_t b0 = (size_t)w * B + (size_t)j * L;
  typename Ar::A R = Ar::zero(), acc = Ar::zero();
  for (int k = (int)L - 1; k >= 0; --k) {
    R = Ar::add(R, Ar::load(bucket_sum, b0 + k));
    acc = Ar::add(acc, R);
  }
  acc = Ar::add(acc, small_mul_ar<Ar>(R, j * L));
  Ar::store(out, t, acc);
}

// Two-level window sums with one lane per point (the pair kernels below
// explain the scheme): level 1 A_j, R_j per L1-bucket segment without fix-up,
// level 2 sum_j j R_j with 0-based weights, out = sum_j A_j + L1 sum_j j R_j.
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, AccWaves<Curve>::value) void window_seg1_kernel(
    const XYZZ<typename Curve::F>* __restrict__ bucket_sum, unsigned W, unsigned B, unsigned L,
    XYZZ<typename Curve::F>* __restrict__ out_a, XYZZ<typename Curve::F>* __restrict__ out_r) {
  const uint32_t S = B / L;
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= W * S) return;
  const uint32_t w = t / S, j = t - w * S;
  const size_t b0 = (size_t)w * B + (size_t)j * L;
  typename Ar::A R = Ar::zero(), acc = Ar::zero();
  for (int k = (int)L - 1; k >= 0; --k) {
    R = Ar::add(R, Ar::load(bucket_sum, b0 + k));
    acc = Ar::add(acc, R);
  }
  Ar::store(out_a, t, acc);
  Ar::store(out_r, t, R);
}
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, AccWaves<Curve>::value) void window_seg2_kernel(
    const XYZZ<typename Curve::F>* __restrict__ in, unsigned W, unsigned S, unsigned L2,
    XYZZ<typename Curve::F>* __restrict__ out) {
  const uint32_t S2 = S / L2;
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= W * S2) return;
  const uint32_t w = t / S2, q = t - w * S2;
  const size_t b0 = (size_t)w * S + (size_t)q * L2;
  typename Ar::A R = Ar::zero(), acc = Ar::zero();
  for (int k = (int)L2 - 1; k >= 0; --k) {  // acc before R: weights k, not k + 1
    acc = Ar::add(acc, R);
    R = Ar::add(R, Ar::load(in, b0 + k));
  }
  acc = Ar::add(acc, small_mul_ar<Ar>(R, q * L2));
  Ar::store(out, t, acc);
}
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, AccWaves<Curve>::value) void window_combine_kernel(
    const XYZZ<typename Curve::F>* __restrict__ a, const XYZZ<typename Curve::F>* __restrict__ b, unsigned W,
    unsigned m, XYZZ<typename Curve::F>* __restrict__ out) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= W) return;
  Ar::store(out, t, Ar::add(Ar::load(a, t), small_mul_ar<Ar>(Ar::load(b, t), m)));
}

// (BLS12-381's limb pair spills here at the two-wave cap; one wave per SIMD
// without spills measured slower: reduction 14.1 -> 14.7 ms at 2^24,
// profiles/r04b/ab_window_segment_one_wave_rejected.log)
template <class Curve, class Ar = FipsPairArith<Curve>>
#ifndef TACHYON_SEG_PAIR_WAVES
#define TACHYON_SEG_PAIR_WAVES 2  // (A/B builds: 1 lifts the VGPR cap that makes the BLS12-381 G2 segment sums spill)
#endif
__global__ __launch_bounds__(kBlock, TACHYON_SEG_PAIR_WAVES) void window_segment_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ bucket_sum,
                                                                     unsigned W, unsigned B, unsigned L,
                                                                     XYZZ<typename Curve::F>* __restrict__ out) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t S = B / L;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W * S) return;
  const uint32_t w = t / S, j = t - w * S;
  const Fb* bs = reinterpret_cast<const Fb*>(bucket_sum);
  const size_t b0 = (size_t)w * B + (size_t)j * L;
  typename Ar::A R = Ar::zero(h != 0), acc = R;
  for (int k = (int)L - 1; k >= 0; --k) {
    R = Ar::add(R, Ar::load(bs, b0 + k, h), h != 0);
    acc = Ar::add(acc, R, h != 0);
  }
  acc = Ar::add(acc, Ar::small_mul(R, j * L, h != 0), h != 0);
  Ar::store(reinterpret_cast<Fb*>(out), t, h, acc);
}

// Two-level window sums (G2 lane pairs, round 5).  sum_b (b + 1) B_b over a
// window's B buckets in segments of L1: level 1 gives each segment j its local
// weighted sum A_j = sum_k (k + 1) B_{j L1 + k} and plain sum R_j with no
// (j L1) R_j fix-up; level 2 prices all fix-ups at once, sum_j j R_j, by the
// same running sums over the R_j (0-based weights, segments of L2 with the
// small fix-up of the one-level kernel); the window is sum_j A_j + L1 sum_j j
// R_j.  Per bucket ~2 + 3 / L1 additions instead of 2 + (the ~log2(B)
// doublings and adds of a fix-up) / L, and with L1 = 16 four times the threads
// of L = 64.  Measured slower (set_variant bit 23, see
// MsmGpu::window_sums_two_level): the trees over the partial sums add more than the fix-ups cost.
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, 2) void window_seg1_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ bucket_sum,
                                                                  unsigned W, unsigned B, unsigned L,
                                                                  XYZZ<typename Curve::F>* __restrict__ out_a,
                                                                  XYZZ<typename Curve::F>* __restrict__ out_r) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t S = B / L;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W * S) return;
  const uint32_t w = t / S, j = t - w * S;
  const Fb* bs = reinterpret_cast<const Fb*>(bucket_sum);
  const size_t b0 = (size_t)w * B + (size_t)j * L;
  typename Ar::A R = Ar::zero(h != 0), acc = R;
  for (int k = (int)L - 1; k >= 0; --k) {
    R = Ar::add(R, Ar::load(bs, b0 + k, h), h != 0);
    acc = Ar::add(acc, R, h != 0);
  }
  Ar::store(reinterpret_cast<Fb*>(out_a), t, h, acc);
  Ar::store(reinterpret_cast<Fb*>(out_r), t, h, R);
}
// level 2: out[w S2 + q] = sum_{k < L2} (q L2 + k) R_{w S + q L2 + k}
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, 2) void window_seg2_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ in,
                                                                  unsigned W, unsigned S, unsigned L2,
                                                                  XYZZ<typename Curve::F>* __restrict__ out) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t S2 = S / L2;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W * S2) return;
  const uint32_t w = t / S2, q = t - w * S2;
  const Fb* src = reinterpret_cast<const Fb*>(in);
  const size_t b0 = (size_t)w * S + (size_t)q * L2;
  typename Ar::A R = Ar::zero(h != 0), acc = R;
  for (int k = (int)L2 - 1; k >= 0; --k) {  // acc before R: weights k, not k + 1
    acc = Ar::add(acc, R, h != 0);
    R = Ar::add(R, Ar::load(src, b0 + k, h), h != 0);
  }
  acc = Ar::add(acc, Ar::small_mul(R, q * L2, h != 0), h != 0);
  Ar::store(reinterpret_cast<Fb*>(out), t, h, acc);
}
// out[w] = a[w] + m b[w]
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, 2) void window_combine_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ a,
                                                                     const XYZZ<typename Curve::F>* __restrict__ b,
                                                                     unsigned W, unsigned m,
                                                                     XYZZ<typename Curve::F>* __restrict__ out) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W) return;
  const typename Ar::A x = Ar::load(reinterpret_cast<const Fb*>(a), t, h);
  const typename Ar::A y = Ar::load(reinterpret_cast<const Fb*>(b), t, h);
  Ar::store(reinterpret_cast<Fb*>(out), t, h, Ar::add(x, Ar::small_mul(y, m, h != 0), h != 0));
}

// The window segment sums in two passes (G2 lane pairs, set_variant bit 24):
// window_segment_pair_kernel holds R, the running sum and a loaded bucket
// (three G2 points, ~540 VGPRs of state for BLS12-381, spilled at the
// two-wave cap).  Pass 1 keeps R and the loaded bucket only and stores every
// suffix sum R_k = sum_{k' >= k} B_{j L + k'} of its segment; pass 2 sums a
// segment's stored R_k (the running sum's value), pass 3 adds the (j L) R_0
// fix-up -- the same segment sums, with two points live in each loop.
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, 2) void window_rsum_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ bucket_sum,
                                                                  unsigned W, unsigned B, unsigned L,
                                                                  XYZZ<typename Curve::F>* __restrict__ rs) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t S = B / L;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W * S) return;
  const uint32_t w = t / S, j = t - w * S;
  const Fb* bs = reinterpret_cast<const Fb*>(bucket_sum);
  Fb* out = reinterpret_cast<Fb*>(rs);
  const size_t b0 = (size_t)w * B + (size_t)j * L;
  typename Ar::A R = Ar::zero(h != 0);
  for (int k = (int)L - 1; k >= 0; --k) {
    R = Ar::add(R, Ar::load(bs, b0 + k, h), h != 0);
    Ar::store(out, b0 + k, h, R);
  }
}
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, 2) void window_rsum_total_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ rs,
                                                                        unsigned W, unsigned B, unsigned L,
                                                                        XYZZ<typename Curve::F>* __restrict__ out) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t S = B / L;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W * S) return;
  const uint32_t w = t / S, j = t - w * S;
  const Fb* src = reinterpret_cast<const Fb*>(rs);
  const size_t b0 = (size_t)w * B + (size_t)j * L;
  typename Ar::A acc = Ar::load(src, b0, h);
  for (uint32_t k = 1; k < L; ++k) acc = Ar::add(acc, Ar::load(src, b0 + k, h), h != 0);
  Ar::store(reinterpret_cast<Fb*>(out), t, h, acc);
}
// pass 3: the (j L) R_0 fix-ups, out[t] += (j L) rs[segment start] (apart,
// so the summing loop above keeps the scalar multiplication's registers free)
template <class Curve, class Ar>
__global__ __launch_bounds__(kBlock, 2) void window_rsum_fix_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ rs,
                                                                      unsigned W, unsigned B, unsigned L,
                                                                      XYZZ<typename Curve::F>* __restrict__ out) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t S = B / L;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W * S) return;
  const uint32_t w = t / S, j = t - w * S;
  if (j == 0) return;  // (both lanes of the pair)
  const typename Ar::A fix = Ar::small_mul(Ar::load(reinterpret_cast<const Fb*>(rs), (size_t)w * B + (size_t)j * L, h),
                                           j * L, h != 0);
  Fb* o = reinterpret_cast<Fb*>(out);
  Ar::store(o, t, h, Ar::add(Ar::load(o, t, h), fix, h != 0));
}

template <class Curve, class Ar = FipsPairArith<Curve>>
__global__ __launch_bounds__(kBlock, 2) void reduce_uniform_pair_kernel(const XYZZ<typename Curve::F>* __restrict__ in,
                                                                     unsigned W, unsigned S_in, unsigned K2,
                                                                     XYZZ<typename Curve::F>* __restrict__ out) {
  using Fb = typename Ar::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const uint32_t S_out = (S_in + K2 - 1) / K2;
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) >> 1;
  if (t >= W * S_out) return;
  const uint32_t w = t / S_out, q = t - w * S_out;
  const uint32_t e0 = q * K2, e1 = min(S_in, e0 + K2);
  const Fb* src = reinterpret_cast<const Fb*>(in) + (size_t)8 * w * S_in;
  typename Ar::A acc = Ar::load(src, e0, h);
  for (uint32_t e = e0 + 1; e < e1; ++e) acc = Ar::add(acc, Ar::load(src, e, h), h != 0);
  Ar::store(reinterpret_cast<Fb*>(out), t, h, acc);
}

// BN254 G1 over the 29-bit field (see seg_reduce29_kernel, msm_join.h).
// One pass over the windows of both widths: windows [0, narrow) have B
// buckets, windows [narrow, W) 2 B (MsmPlan::make_mixed; the uniform plan is
// narrow = W).  L divides B, so the segments tile the concatenated bucket
// array: thread t owns buckets [t L, (t + 1) L), segment j of its window by
// the closed forms of recode_scalar / bucket_of_key, and the segment sums come
// out window-major (S = B / L per narrow window, 2 S per wide one).  The load
// of bucket k - 1 is issued before the two additions of bucket k: at two waves
// per SIMD nothing else hides the 144-byte gather.
template <bool kRaw>
__global__ __launch_bounds__(kBlock, 2) void window_segment29_kernel(const XYZZ<Bn254Fq>* __restrict__ bucket_sum,
                                                                    unsigned W, unsigned narrow, unsigned B, unsigned L,
                                                                    XYZZ<Bn254Fq>* __restrict__ out) {
  const uint32_t S = B / L;
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lo = narrow * S;  // segments of the narrow windows
  if (t >= lo + (W - narrow) * 2 * S) return;
  const uint32_t j = t < lo ? t % S : (t - lo) % (2 * S);
  const size_t b0 = (size_t)t * L;
  auto load = [&](size_t i) { return kRaw ? acc29::load_raw(bucket_sum, i) : acc29::load_pt(bucket_sum, i); };
  acc29::Pt R{acc29::Acc{}, true}, acc = R;
  acc29::Pt next = load(b0 + L - 1);
  for (int k = (int)L - 1; k >= 0; --k) {
    const acc29::Pt cur = next;
    if (k > 0) next = load(b0 + k - 1);
    R = acc29::add(R, cur);
    acc = acc29::add(acc, R);
  }
  acc = acc29::add(acc, acc29::small_mul(R, j * L));
  acc29::store_pt(out, t, acc);
}
// The last levels of the window sums in ONE launch per MSM: workgroup w
// reduces window w's S <= kBlock segment sums by a binary tree through LDS
// (log2 S dependent additions, as the one-launch-per-level binary tree,
// without a launch per level: 2^16 has S = 64 -> 6 launches of ~12 us, each
// mostly one latency-bound addition).  (Computing the segment sums in this
// kernel too, window_segment29_kernel's loop, gave wrong window sums on the
// GPU although the loop is the same code -- not understood, so not used.)
__global__ __launch_bounds__(kBlock, 2) void window_tree29_kernel(const XYZZ<Bn254Fq>* __restrict__ in, unsigned narrow,
                                                                 unsigned S, XYZZ<Bn254Fq>* __restrict__ out) {
  __shared__ acc29::Raw sh[kBlock];
  const uint32_t w = blockIdx.x, j = threadIdx.x;
  // window w's sums: S of them below `narrow`, 2 S from there on (window_segment29_kernel)
  const uint32_t Sw = w < narrow ? S : 2 * S;
  const size_t first = w < narrow ? (size_t)w * S : (size_t)narrow * S + (size_t)(w - narrow) * 2 * S;
  acc29::Pt v{acc29::Acc{}, true};
  if (j < Sw) v = acc29::load_pt(in, first + j);
  unsigned span = 1;
  while (span < Sw) span <<= 1;
  for (unsigned half = span >> 1; half >= 1; half >>= 1) {
    if (j >= half && j < 2 * half) acc29::store_raw(sh, j - half, v);
    __syncthreads();
    if (j < half) v = acc29::add(v, acc29::load_raw(sh, j));
    __syncthreads();
  }
  if (j == 0) acc29::store_pt(out, w, v);
}
// window_segment29 + window_tree29 in one launch (S = B / L <= kBlock segment
// sums per window): thread j of workgroup w computes segment j's sum exactly
// as window_segment29_kernel does, then the LDS tree.  Every thread reaches
// every barrier (no early return).  set_variant bit 19 (A/B).
template <bool kRaw>
__global__ __launch_bounds__(kBlock, 2) void window_segtree29_kernel(const XYZZ<Bn254Fq>* __restrict__ bucket_sum,
                                                                    unsigned B, unsigned L,
                                                                    XYZZ<Bn254Fq>* __restrict__ out) {
  __shared__ acc29::Raw sh[kBlock];
  const uint32_t S = B / L;
  const uint32_t w = blockIdx.x, j = threadIdx.x;
  acc29::Pt v{acc29::Acc{}, true};
  if (j < S) {
    const size_t b0 = (size_t)w * B + (size_t)j * L;
    acc29::Pt R{acc29::Acc{}, true};
    v = R;
    for (int k = (int)L - 1; k >= 0; --k) {
      R = acc29::add(R, kRaw ? acc29::load_raw(bucket_sum, b0 + k) : acc29::load_pt(bucket_sum, b0 + k));
      v = acc29::add(v, R);
    }
    v = acc29::add(v, acc29::small_mul(R, j * L));
  }
  unsigned span = 1;
  while (span < S) span <<= 1;
  for (unsigned half = span >> 1; half >= 1; half >>= 1) {
    if (j >= half && j < 2 * half) acc29::store_raw(sh, j - half, v);
    __syncthreads();
    if (j < half) v = acc29::add(v, acc29::load_raw(sh, j));
    __syncthreads();
  }
  if (j == 0) acc29::store_pt(out, w, v);
}

// Window sums of windows with B <= kBlock buckets (c <= 9: the 2^16 MSM) in
// one launch, workgroup w = window w: sum_b (b + 1) B_b = sum_k T_k with the
// suffix sums T_k = sum_{b >= k} B_b, by a Hillis-Steele scan through LDS
// (log2 B levels of one addition) and a binary tree over the T_k (log2 B
// more): 14 dependent additions at B = 128 against window_segment29's L = 2
// running sums plus the (jL) R fix-up (~17) and the tree of the segment sums
// (6), and one launch instead of two.
template <bool kRaw>
__global__ __launch_bounds__(kBlock, 2) void window_scan29_kernel(const XYZZ<Bn254Fq>* __restrict__ bucket_sum,
                                                                 unsigned B, XYZZ<Bn254Fq>* __restrict__ out) {
  __shared__ acc29::Raw sh[kBlock];
  const uint32_t w = blockIdx.x, j = threadIdx.x;
  acc29::Pt v{acc29::Acc{}, true};
  if (j < B) v = kRaw ? acc29::load_raw(bucket_sum, (size_t)w * B + j) : acc29::load_pt(bucket_sum, (size_t)w * B + j);
  for (unsigned d = 1; d < B; d <<= 1) {  // v = T_j
    acc29::store_raw(sh, j, v);
    __syncthreads();
    if (j + d < B) v = acc29::add(v, acc29::load_raw(sh, j + d));
    __syncthreads();
  }
  unsigned span = 1;
  while (span < B) span <<= 1;
  for (unsigned half = span >> 1; half >= 1; half >>= 1) {
    if (j >= half && j < 2 * half) acc29::store_raw(sh, j - half, v);
    __syncthreads();
    if (j < half) v = acc29::add(v, acc29::load_raw(sh, j));
    __syncthreads();
  }
  if (j == 0) acc29::store_pt(out, w, v);
}

// (windows [0, narrow) hold S_in sums each, windows [narrow, W) 2 S_in, in and
// out window-major as window_segment29_kernel writes them)
__global__ __launch_bounds__(kBlock, 2) void reduce_uniform29_kernel(const XYZZ<Bn254Fq>* __restrict__ in, unsigned W,
                                                                    unsigned narrow, unsigned S_in, unsigned K2,
                                                                    XYZZ<Bn254Fq>* __restrict__ out) {
  const uint32_t out_lo = (S_in + K2 - 1) / K2, out_hi = (2 * S_in + K2 - 1) / K2;
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lo = narrow * out_lo;
  if (t >= lo + (W - narrow) * out_hi) return;
  uint32_t q, S;
  size_t first;
  if (t < lo) {
    const uint32_t w = t / out_lo;
    q = t - w * out_lo, S = S_in, first = (size_t)w * S_in;
  } else {
    const uint32_t w = (t - lo) / out_hi;
    q = (t - lo) - w * out_hi, S = 2 * S_in, first = (size_t)narrow * S_in + (size_t)w * 2 * S_in;
  }
  const uint32_t e0 = q * K2, e1 = min(S, e0 + K2);
  const XYZZ<Bn254Fq>* src = in + first;
  acc29::Pt acc = acc29::load_pt(src, e0);
  for (uint32_t e = e0 + 1; e < e1; ++e) acc = acc29::add(acc, acc29::load_pt(src, e));
  acc29::store_pt(out, t, acc);
}

// Window reduction, stage 2: sum K2 consecutive segment sums per window.
template <class Curve, class Ar = FipsArith<Curve>>
__global__ __launch_bounds__(kBlock, AccWaves<Curve>::value) void reduce_uniform_kernel(const XYZZ<typename Curve::F>* __restrict__ in,
                                                                unsigned W, unsigned S_in, unsigned K2,
                                                                XYZZ<typename Curve::F>* __restrict__ out) {
  uint32_t S_out = (S_in + K2 - 1) / K2;
  uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= W * S_out) return;
  uint32_t w = t / S_out, q = t - w * S_out;
  uint32_t e0 = q * K2, e1 = min(S_in, e0 + K2);
  const XYZZ<typename Curve::F>* src = in + (size_t)w * S_in;
  typename Ar::A acc = Ar::load(src, e0);
  for (uint32_t e = e0 + 1; e < e1; ++e) acc = Ar::add(acc, Ar::load(src, e));
  Ar::store(out, t, acc);
}

// Window reduction by workgroup trees (no per-segment (jL)*R fix-up, two
// launches instead of one per binary-tree level).  Units of a window are
// segments of L buckets; a node over the units [a, a + s) is
//   V  = sum_j [A_j + (j - a) L R_j],   Rs = s L sum_j R_j
// (A_j = sum_k (k + 1) B_{jL+k}, R_j = sum_k B_{jL+k}: the segment's running
// sums), so the root over all units is the window sum sum_b (b + 1) B_b
// (PippengerBase::AccumulateBuckets, pippenger_base.h:36-57).  Two adjacent
// nodes of equal size merge as V = V_l + V_r + Rs_r, Rs = 2 (Rs_l + Rs_r):
// three point operations per merge, none depending on the position.
// kLeafBuckets: leaves are segments read from bucket_sum (grid (groups, W));
// otherwise leaves are the nodes of the previous launch (`nodes_in`, `units`
// per window).  Each workgroup writes the node over its kWinBlock leaves
// (padding leaves are (0, 0): units past the end hold no buckets).
constexpr unsigned kWinBlock = 256;
template <class Curve, bool kLeafBuckets>
__global__ __launch_bounds__(kWinBlock, AccWaves<Curve>::value) void window_tree_kernel(
    const XYZZ<typename Curve::F>* __restrict__ bucket_sum, unsigned B, unsigned L, unsigned log_l,
    const XYZZ<typename Curve::F>* __restrict__ nodes_in, unsigned units, XYZZ<typename Curve::F>* __restrict__ nodes_out) {
  using F = typename HotOf<typename Curve::F>::type;
  using P = XYZZ<F>;
  extern __shared__ uint64_t win_lds[];
  P* lv = reinterpret_cast<P*>(win_lds);           // kWinBlock / 2 right-node V
  P* lr = lv + kWinBlock / 2;                      // and Rs
  const unsigned t = threadIdx.x, w = blockIdx.y;
  const unsigned u = blockIdx.x * kWinBlock + t;   // this thread's leaf unit
  P V = P::zero(), Rs = P::zero();
  if (u < units) {
    if constexpr (kLeafBuckets) {
      const P* bs = reinterpret_cast<const P*>(bucket_sum) + (size_t)w * B + (size_t)u * L;
      for (int k = (int)L - 1; k >= 0; --k) {
        Rs = Rs + bs[k];
        V = V + Rs;
      }
      for (unsigned k = 0; k < log_l; ++k) Rs = Rs.dbl();  // L R
    } else {
      const P* in = reinterpret_cast<const P*>(nodes_in) + 2 * ((size_t)w * units + u);
      V = in[0];
      Rs = in[1];
    }
  }
  for (unsigned k = 0; (1u << k) < kWinBlock; ++k) {
    const unsigned span = 1u << k;
    if ((t & (2 * span - 1)) == span) {  // a right node: hand it to its left neighbour
      lv[t >> (k + 1)] = V;
      lr[t >> (k + 1)] = Rs;
    }
    __syncthreads();
    if ((t & (2 * span - 1)) == 0) {
      const P rv = lv[t >> (k + 1)], rr = lr[t >> (k + 1)];
      V = V + rv + rr;
      Rs = (Rs + rr).dbl();
    }
    __syncthreads();
  }
  if (t == 0) {
    const unsigned groups = gridDim.x;
    P* o = reinterpret_cast<P*>(nodes_out) + 2 * ((size_t)w * groups + blockIdx.x);
    o[0] = V;
    o[1] = Rs;
  }
}

}  // namespace
}  // namespace detail
}  // namespace tachyon_amd::msm
