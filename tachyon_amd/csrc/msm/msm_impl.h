// Variable-base MSM kernels for MI355X (gfx950) and their host driver
// (template definitions; one translation unit per curve instantiates them:
// msm_bn254_g1.hip, msm_bn254_g2.hip, msm_bls12_381_g1.hip, msm_bls12_381_g2.hip).
// See msm.h for the pipeline; reference semantics: pippenger.h:28-170,
// pippenger_base.h:36-77 (the answer is the same group element; the parity
// tests compare affine coordinates bytewise).
#pragma once
#include "msm.h"
#include "../field/f29.h"
#include "acc29.h"
#include "acc28.h"
#include "acc_pair.h"
#include "pair28.h"
#include "pair29.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>

namespace tachyon_amd::msm {

namespace detail {
namespace {  // internal linkage: every per-curve TU gets its own copy

constexpr unsigned kBlock = 256;
constexpr uint32_t kSignBit = 0x80000000u;
constexpr uint32_t kNoBucket = 0xFFFFFFFFu;
enum : uint32_t { kHead = 1, kTail = 2, kSingle = 4 };

}  // namespace
}  // namespace detail
}  // namespace tachyon_amd::msm

// the kernels, stage by stage (each header keeps the detail / anonymous-namespace arrangement)
#include "msm_recode.h"
#include "msm_bases.h"
#include "msm_acc.h"
#include "msm_join.h"
#include "msm_window.h"
#include "msm_sort.h"

namespace tachyon_amd::msm {

namespace detail {
namespace {

inline unsigned grid_for(size_t threads) { return (unsigned)std::max<size_t>(1, (threads + kBlock - 1) / kBlock); }

}  // namespace
}  // namespace detail
using namespace detail;

template <class Curve>
MsmGpu<Curve>::MsmGpu(hipStream_t stream) : stream_(stream) {
  require_gpu();
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  for (auto& e : ev_) TA_HIP(hipEventCreate(&e));
  TA_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_max_), 2 * sizeof(uint32_t), hipHostMallocDefault));
}

template <class Curve>
MsmGpu<Curve>::~MsmGpu() {
  for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
  for (auto* v : {&gev_sorted_, &gev_acc0_, &gev_acc1_})
    for (auto& e : *v) (void)hipEventDestroy(e);
  if (sort_stream_) (void)hipStreamDestroy(sort_stream_);
  if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
  if (copy_done_) (void)hipEventDestroy(copy_done_);
  for (auto e : chunk_ev_) (void)hipEventDestroy(e);
  if (h_max_) (void)hipHostFree(h_max_);
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

template <class Curve>
void MsmGpu<Curve>::ensure_group_events(unsigned groups) {
  while (gev_sorted_.size() < groups) {
    hipEvent_t a, b, c;
    TA_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
    TA_HIP(hipEventCreate(&b));
    TA_HIP(hipEventCreate(&c));
    gev_sorted_.push_back(a);
    gev_acc0_.push_back(b);
    gev_acc1_.push_back(c);
  }
}

template <class Curve>
hipError_t MsmGpu<Curve>::sort_entries(void* tmp, size_t& bytes, const uint64_t* in, uint64_t* out, size_t count,
                                       unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  begin_bit += 32;
  end_bit += 32;
  switch (sort_cfg_) {
    case 1:
      return rocprim::radix_sort_keys(tmp, bytes, in, out, count, begin_bit, end_bit, s);
    case 2:
      return rocprim::radix_sort_keys<OnesweepCfg<512, 16>>(tmp, bytes, in, out, count, begin_bit, end_bit, s);
    case 3:
      return rocprim::radix_sort_keys<OnesweepCfg<1024, 12>>(tmp, bytes, in, out, count, begin_bit, end_bit, s);
    default:
      return rocprim::radix_sort_keys<OnesweepCfg<1024, 8>>(tmp, bytes, in, out, count, begin_bit, end_bit, s);
  }
}

// ---------------------------------------------------------------------------
// enqueue() and its stages.  Shape is what the run covers, derived once from
// the plan and the context's batch / fold state (make_shape); Buffers the
// device pointers cut from the DeviceBuffers for it (carve).  Both are passed
// by const reference.
template <class Curve>
struct MsmGpu<Curve>::Shape {
  size_t n;
  // Ws = the windows each scalar emits (plan.active()); Wt = all windows of
  // the scalar (the recode's carry chain), the range starting at window
  // w_begin; W = the window sums this run computes (make_shape)
  unsigned Ws, Wt, w_begin, W, B, c;
  // mixed widths (MsmPlan::make_mixed): windows [narrow, W) are c + 1 bits wide
  // with 2 B buckets, keys are bucket indices; uniform: narrow = ~0u.  key_c is
  // what bucket_of_key decodes the keys by (c, or 0 for the mixed keys)
  bool mixed;
  uint32_t narrow;
  unsigned key_c;
  uint32_t K;
  unsigned K2, seg, seg_tree;  // the plan's join fan-in and window-sum segment lengths
  unsigned G, ngroups;
  size_t epw;      // entries per key window's share of the array (n without a batch)
  size_t T;        // accumulation threads over all groups
  size_t entries;  // n * Ws
  size_t nb;       // W * B buckets (mixed widths: narrow * B + (W - narrow) * 2 B)
  uint32_t fold_w, glen, gstep, fold_n;  // recode_scalar's batch / fold arguments
  SlotBytes sb;
  SortShape ss;
  ChainMode chain_mode;
  unsigned lv_max;  // kChainsInStream: the bound of the join levels whose offsets are built early
};

template <class Curve>
struct MsmGpu<Curve>::Buffers {
  hipStream_t sort_stream;
  uint64_t *ents, *ents2;
  Point *bucket_sum, *pieces, *lvl_buf;
  uint32_t* early_ltab;       // kChainsInStream: every join level's offsets
  uint32_t *tflags, *tlast;   // the accumulation's run flags and last buckets
  uint32_t *cflags, *clast;   // what the chain kernels read
  uint32_t *is_start, *cid;
  uint32_t *cbeg, *cend, *cbucket, *lcnt;  // chain tables: beg, end, bucket, level counts/offsets (<= T chains)
  uint32_t* dscal;            // [0] nchains, [1] max chain length
  void* sort_tmp;             // rocPRIM's radix sort scratch, sort_bytes of it
  size_t sort_bytes;
  uint8_t* os_tmp;            // own passes: lookback states, block id, spare offsets
  size_t lookback_bytes;
};

// The reduction kernels of a run (chain join and window sums): one table per
// run, from the curve, the field code, `raw` and the variant bits.
template <class Curve>
struct MsmGpu<Curve>::ReduceKernels {
  using Level = void (*)(const Point*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, unsigned, Point*,
                         const uint32_t*, Point*);
  using Seg = void (*)(const Point*, unsigned, unsigned, unsigned, Point*);
  using Seg1 = void (*)(const Point*, unsigned, unsigned, unsigned, Point*, Point*);
  using Comb = void (*)(const Point*, const Point*, unsigned, unsigned, Point*);
  unsigned lanes;      // threads per point
  Level level[2][2];   // join level kernel, [first level][last level]
  Seg win_segment, win_reduce;
  Seg rsum_pass1, rsum_pass2, rsum_fix;  // G2 two-pass sums (bit 24)
  Seg1 seg1;                             // two-level window sums (bit 23)
  Seg seg2;
  Comb comb;
};

// The accumulation kernel of one group: kernel, threads per accumulation
// thread (1, or 2 for the lane pairs) and its kSched* bits.
template <class Curve>
struct MsmGpu<Curve>::AccLaunch {
  void (*kernel)(const Aff*, const uint64_t*, uint32_t, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t, Point*,
                 Point*, uint32_t*, uint32_t*);
  unsigned lanes, sched;
};

template <class Curve>
typename MsmGpu<Curve>::Shape MsmGpu<Curve>::make_shape(size_t n, const MsmPlan& plan) const {
  Shape s;
  s.n = n;
  s.Ws = plan.active(), s.Wt = plan.windows, s.w_begin = plan.w_begin, s.B = plan.buckets, s.c = plan.c;
  // W: Ws, or Ws per MSM of a batch over shared bases (run_batch: batch_ MSMs
  // of n / batch_ points each, MSM g's windows g Ws .. g Ws + Ws - 1 in the key
  // space); a fold: Wt / fold_ key windows over fold_ copies of the bases
  // (run_windows checked it)
  s.W = (fold_ > 1 ? s.Wt / fold_ : s.Ws) * batch_;
  s.fold_w = fold_ > 1 ? s.Wt / fold_ : 0u;
  s.glen = batch_ > 1 ? (uint32_t)(n / batch_) : 0u;
  s.gstep = batch_distinct_ ? 0u : s.glen;  // shared bases (run_batch) or one array per MSM (run_groups)
  s.fold_n = s.gstep ? s.glen : (uint32_t)n;  // points per fold copy
  s.entries = n * s.Ws;
  s.mixed = plan.mixed;
  s.narrow = plan.mixed ? plan.narrow() : ~0u;
  s.key_c = plan.mixed ? 0u : s.c;
  s.nb = plan.mixed ? plan.total_buckets() : (size_t)s.W * s.B;
  if (n >= (size_t(1) << 31)) throw std::runtime_error("tachyon_mi355x: MSM size must be < 2^31 per device");
  if (((uint64_t)s.W << s.c) > (uint64_t(1) << 32))  // 32-bit keys (window << c | digit)
    throw std::runtime_error("tachyon_mi355x: too many windows for 32-bit bucket keys (MSM batch too large)");
  s.K = plan.K, s.K2 = plan.K2, s.seg = plan.seg, s.seg_tree = plan.seg_tree;
  // window groups: group g covers windows [g*G, min(W, (g+1)*G)), i.e. the
  // contiguous entry range [w0*n, w1*n); its sort (sort stream) overlaps the
  // accumulation of the previous group (MSM stream) -- the sort is HBM-bound,
  // the accumulation VALU-bound, so they share the CUs well.  A batch or a
  // fold sorts all its windows together: the recode writes the entries by
  // scalar window, not by key window
  s.G = (batch_ > 1 || fold_ > 1) ? s.W : std::max(1u, std::min(plan.group, s.W));
  s.ngroups = (s.W + s.G - 1) / s.G;
  s.epw = s.entries / s.W;
  s.T = 0;
  for (unsigned g = 0; g < s.ngroups; ++g) {
    const unsigned w0 = g * s.G, w1 = std::min(s.W, w0 + s.G);
    s.T += ((size_t)(w1 - w0) * s.epw + s.K - 1) / s.K;
  }
  if (s.T >= (size_t(1) << 31)) throw std::runtime_error("tachyon_mi355x: MSM too large for the chunking");
  // bucket sums, pieces and join levels in the accumulation's raw limb format
  // where the reductions read it (slot_bytes; work_bytes estimates by the same rule)
  s.sb = slot_bytes(acc_, variant_);
  // the sort's shape (sort_shape: work_bytes sizes the sort scratch by the same rule)
  s.ss = sort_shape(sort_, s.c, s.Ws, s.W, s.G, s.entries, s.mixed);
  // Where the chain tables (and the join levels' offsets) are built -- they
  // depend only on the sorted keys (chain_flags_kernel), so they need not wait
  // for the accumulation:
  //  * kChainsInStream: windows with <= 16 K buckets in all (2^16, 2^17):
  //    before the accumulation, with every level's offsets by one workgroup
  //    from the device-side counts (join_offsets_all_kernel); the host reads
  //    the chain count back while the accumulation runs;
  //  * kChainsBefore: other MSMs of < 2^21 accumulation threads: the tables
  //    before the accumulation, the read-back during it, the offsets after;
  //  * kChainsAfter: from the accumulation's flags after it (large MSMs,
  //    where the tables cost more than the read-back gap they hide, and
  //    window-group pipelines).
  // All on the MSM's one stream: a second stream for the tables measured the
  // same alone, but it shifts the process's stream -> hardware-queue
  // round-robin (4 queues), which put the Groth16 prover's G1 and G2 MSM
  // streams on one queue and serialised them (2^20 proof 12.9 -> 14.3 ms,
  // profiles/r03e/ab_groth16_side_stream.log).
  s.chain_mode = s.ngroups != 1                                            ? kChainsAfter
                 : s.nb <= 16384 && s.T < (size_t(1) << 20) ? kChainsInStream
                 : s.T < (size_t(1) << 21)                                 ? kChainsBefore
                                                                           : kChainsAfter;
  s.lv_max = s.chain_mode == kChainsInStream
                 ? join_levels((uint32_t)std::min<size_t>(2 * s.T, ~0u), kJoinFanLong) + 1
                 : 0;
  return s;
}

template <class Curve>
typename MsmGpu<Curve>::Buffers MsmGpu<Curve>::carve(const Shape& s) {
  Buffers b{};
  const size_t T = s.T;
  ensure_group_events(s.ngroups);
  // the sort runs on its own stream only when the windows are pipelined
  // (created on first use: every extra stream may take one of the process's
  // few hardware queues)
  if (s.ngroups > 1 && !sort_stream_) TA_HIP(hipStreamCreateWithFlags(&sort_stream_, hipStreamNonBlocking));
  b.sort_stream = s.ngroups > 1 ? sort_stream_ : stream_;
  // (64 bytes of slack: the LDS-staged entry chunks read up to 7 entries past a lane's last)
  b.ents = static_cast<uint64_t*>(ents_.ensure(s.entries * 8 + 64));
  b.ents2 = static_cast<uint64_t*>(ents2_.ensure(s.entries * 8 + 64));
  b.bucket_sum = static_cast<Point*>(buckets_.ensure(s.nb * s.sb.slot));
  b.pieces = static_cast<Point*>(part_a_.ensure(2 * T * s.sb.slot));
  b.lvl_buf = static_cast<Point*>(part_b_.ensure((2 * T / kJoinFanLong + T + 2) * s.sb.lvl_slot));
  const bool early_chains = s.chain_mode != kChainsAfter;
  b.early_ltab =
      s.chain_mode == kChainsInStream ? static_cast<uint32_t*>(lofs_.ensure(s.lv_max * (T + 2) * 4)) : nullptr;
  b.tflags = static_cast<uint32_t*>(start_.ensure(2 * T * 4));
  b.tlast = static_cast<uint32_t*>(end_.ensure(2 * T * 4));
  b.cflags = early_chains ? b.tflags + T : b.tflags;
  b.clast = early_chains ? b.tlast + T : b.tlast;
  b.is_start = static_cast<uint32_t*>(cnt_.ensure((T + 1) * 4));
  b.cid = static_cast<uint32_t*>(off_a_.ensure((T + 1) * 4));
  uint32_t* ctab = static_cast<uint32_t*>(off_b_.ensure((6 * (T + 2) + 4) * 4));
  b.cbeg = ctab;
  b.cend = ctab + (T + 2);
  b.cbucket = ctab + 2 * (T + 2);
  b.lcnt = ctab + 3 * (T + 2);
  b.dscal = ctab + 6 * (T + 2);
  if (s.ss.own_sort) {
    b.lookback_bytes = (size_t)256 * ((s.entries + kOnesweepMinTile - 1) / kOnesweepMinTile) * 4;
    b.os_tmp = static_cast<uint8_t*>(sort_tmp_.ensure(b.lookback_bytes + 1024 + 256 * 4));
  } else {
    const size_t max_group_entries = (size_t)s.G * s.epw;
    TA_HIP(sort_entries(nullptr, b.sort_bytes, b.ents, b.ents2, max_group_entries, s.ss.sort_begin, s.ss.key_bits,
                        b.sort_stream));
    b.sort_tmp = sort_tmp_.ensure(b.sort_bytes);
  }
  return b;
}

// The fused path with its histogram kernels (which also clear the bucket
// sums), or the plain recode plus the bucket memset.  Returns the global digit
// offsets of the own onesweep passes (nullptr without them).
template <class Curve>
uint32_t* MsmGpu<Curve>::recode(const Shape& s, const Buffers& b, const Fr* d_scalars) {
  const SortShape& ss = s.ss;
  const uint32_t n = (uint32_t)s.n, spt = ss.spt;
  uint32_t* digit_off = nullptr;
  if (ss.fused) {
    const uint32_t nblocks = (uint32_t)((s.n + spt * kBlock - 1) / (spt * kBlock));
    const size_t hn = (size_t)256 * nblocks;
    const unsigned later_places = ss.own_sort ? ss.places : 0;
    // slot chunks: <= 1024 chunks of >= 4 blocks (bin_chunk_scan_kernel's loop, bin_offsets_kernel's rows)
    const uint32_t bper = std::max<uint32_t>(4, (nblocks + 1023) / 1024), bchunks = (nblocks + bper - 1) / bper;
    uint32_t* hist = static_cast<uint32_t*>(
        hist_.ensure(((2 + later_places) * hn + 5 * 256 + 2 * (size_t)bchunks * 256 + 256) * 4));
    uint32_t* hoff = hist + hn;
    uint32_t* later = hist + 2 * hn;
    uint32_t* digit_cnt = later + later_places * hn;  // 2 x 256 counts, 2 x 256 offsets, 256 spare
    uint32_t* bcsum = digit_cnt + 5 * 256;            // [chunk][bin] sums, then prefixes, then the bin totals
    uint32_t* bcpre = bcsum + (size_t)bchunks * 256;
    uint32_t* btotal = bcpre + (size_t)bchunks * 256;
    hipLaunchKernelGGL(recode_hist_kernel<Fr>, dim3(nblocks), dim3(kBlock), 0, stream_, d_scalars, n, s.c, s.Wt,
                       s.w_begin, s.Ws, nblocks, spt, later_places, hist, later, reinterpret_cast<uint4*>(b.bucket_sum),
                       s.nb * s.sb.slot / 16, s.glen, s.gstep, s.fold_w, s.fold_n, s.narrow);
    TA_HIP(hipGetLastError());
    if (later_places > 0) {
      digit_off = digit_cnt + 2 * 256;
      TA_HIP(hipMemsetAsync(digit_cnt, 0, 2 * 256 * 4, stream_));
      // (>= 256 chunks: a 2^16 MSM's 128 recode blocks in one chunk took 17 us of serial loads)
      const uint32_t per_chunk = std::clamp<uint32_t>(nblocks / 256, 4, 128), chunks = (nblocks + per_chunk - 1) / per_chunk;
      hipLaunchKernelGGL(digit_count_kernel, dim3(chunks, later_places), dim3(kBlock), 0, stream_, later, nblocks,
                         per_chunk, digit_cnt);
      hipLaunchKernelGGL(digit_scan_kernel, dim3(later_places), dim3(kBlock), 0, stream_, digit_cnt, digit_off);
      TA_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bin_chunk_sums_kernel, dim3(bchunks), dim3(kBlock), 0, stream_, hist, nblocks, bper, bcsum);
    hipLaunchKernelGGL(bin_chunk_scan_kernel, dim3(256), dim3(kBlock), 0, stream_, bcsum, bchunks, bcpre, btotal);
    hipLaunchKernelGGL(bin_offsets_kernel, dim3(bchunks), dim3(kBlock), 0, stream_, hist, nblocks, bper, bcpre, btotal,
                       hoff);
    TA_HIP(hipGetLastError());
    // the scattered entries are fully sorted when the key has <= 8 bits; the
    // own onesweep passes ping-pong from the scatter's output and end in ents2
    uint64_t* dst = ss.own_sort ? (ss.places % 2 == 0 ? b.ents2 : b.ents) : (ss.sort_begin < ss.key_bits ? b.ents : b.ents2);
    auto* scatter = ss.narrow ? &recode_scatter_kernel<Fr, true> : &recode_scatter_kernel<Fr, false>;
    // dynamic LDS above 64 KiB: raise the launched instance's limit once (per instantiation)
    if (ss.scatter_lds > 64 * 1024 && !scatter_lds_set_[ss.narrow ? 1 : 0]) {
      TA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(scatter), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 128 * 1024));
      scatter_lds_set_[ss.narrow ? 1 : 0] = true;
    }
    hipLaunchKernelGGL(scatter, dim3(nblocks), dim3(kBlock), ss.scatter_lds, stream_, d_scalars, n, s.c, s.Wt,
                       s.w_begin, s.Ws, nblocks, spt, hist, hoff, dst, s.glen, s.gstep, s.fold_w, s.fold_n, s.narrow);
  } else {
    hipLaunchKernelGGL(recode_kernel<Fr>, dim3(grid_for(s.n)), dim3(kBlock), 0, stream_, d_scalars, n, s.c, s.Wt,
                       s.w_begin, s.Ws, b.ents, s.glen, s.gstep, s.fold_w, s.fold_n, s.narrow);
  }
  TA_HIP(hipGetLastError());
  // every bucket without an entry stays the identity (the fused recode clears them)
  if (!ss.fused) TA_HIP(hipMemsetAsync(b.bucket_sum, 0, s.nb * s.sb.slot, stream_));
  return digit_off;
}

// Radix sort of group g's (window, bucket, point) entries [e0, e0 + ecount)
// into ents2, on the sort stream; the MSM stream waits for it.
template <class Curve>
void MsmGpu<Curve>::sort_group(const Shape& s, const Buffers& b, unsigned g, size_t e0, size_t ecount,
                               uint32_t* digit_off) {
  const SortShape& ss = s.ss;
  if (ss.own_sort) {
    const uint64_t* src = ss.places % 2 == 0 ? b.ents2 : b.ents;
    uint64_t* out = ss.places % 2 == 0 ? b.ents : b.ents2;
    for (unsigned q = 0; q < ss.places; ++q) {
      TA_HIP(onesweep_pass(sort_cfg_, src, out, (uint32_t)s.entries, 32 + ss.sort_begin + 8 * q, 32 + ss.key_bits,
                           digit_off + q * 256, reinterpret_cast<uint32_t*>(b.os_tmp + b.lookback_bytes + 1024),
                           b.os_tmp, b.os_tmp + b.lookback_bytes, b.sort_stream));
      src = out;
      out = out == b.ents ? b.ents2 : b.ents;
    }
  } else if (ss.sort_begin < ss.key_bits) {
    size_t bytes = b.sort_bytes;
    TA_HIP(sort_entries(b.sort_tmp, bytes, b.ents + e0, b.ents2 + e0, ecount, ss.sort_begin, ss.key_bits,
                        b.sort_stream));
  }
  if (profile_ && g + 1 == s.ngroups) TA_HIP(hipEventRecord(ev_[kMarkSorted], b.sort_stream));  // last sort done
  if (b.sort_stream != stream_) {
    TA_HIP(hipEventRecord(gev_sorted_[g], b.sort_stream));
    TA_HIP(hipStreamWaitEvent(stream_, gev_sorted_[g], 0));
  }
}

// host-resident bases: their upload (the larger of the two) runs on its
// own stream while the recode and the sort run; the host call returns
// once the pageable copy is staged, i.e. with the GPU busy meanwhile
template <class Curve>
void MsmGpu<Curve>::upload_pending_bases(const Aff* d_bases, size_t n) {
  if (!copy_stream_) TA_HIP(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
  if (!copy_done_) TA_HIP(hipEventCreateWithFlags(&copy_done_, hipEventDisableTiming));
  TA_HIP(hipMemcpyAsync(const_cast<Aff*>(d_bases), pending_host_bases_, n * sizeof(Aff), hipMemcpyHostToDevice,
                        copy_stream_));
  TA_HIP(hipEventRecord(copy_done_, copy_stream_));
  TA_HIP(hipStreamWaitEvent(stream_, copy_done_, 0));
  pending_host_bases_ = nullptr;
}

// Chain tables from the per-thread run flags: a chain = the pieces of one
// bucket across consecutive threads (head/tail pieces), numbered by a scan
// of the chain starts; then each chain's first-level piece count, the chain
// count and the longest chain, read back into h_max_ (pinned).
template <class Curve>
void MsmGpu<Curve>::build_chains(const Shape& s, const Buffers& b) {
  const size_t T = s.T;
  hipLaunchKernelGGL(chain_mark_kernel, dim3(grid_for(T + 1)), dim3(kBlock), 0, stream_, b.cflags, (uint32_t)T,
                     b.is_start, b.dscal + 1);
  size_t scan_bytes = 0;
  TA_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, b.is_start, b.cid, 0u, T + 1, rocprim::plus<uint32_t>(), stream_));
  void* scan_tmp = scan_tmp_.ensure(scan_bytes);
  TA_HIP(rocprim::exclusive_scan(scan_tmp, scan_bytes, b.is_start, b.cid, 0u, T + 1, rocprim::plus<uint32_t>(), stream_));
  hipLaunchKernelGGL(chain_build_kernel, dim3(grid_for(T)), dim3(kBlock), 0, stream_, b.cflags, b.clast, b.cid,
                     (uint32_t)T, b.cbeg, b.cend, b.cbucket, b.dscal);
  hipLaunchKernelGGL(seg_count_kernel, dim3(grid_for(T + 1)), dim3(kBlock), 0, stream_, b.cbeg, b.cend, b.dscal,
                     (uint32_t)T, s.K2, b.lcnt, b.dscal + 1);
  TA_HIP(hipGetLastError());
  TA_HIP(hipMemcpyAsync(h_max_, b.dscal, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
}

// kChainsInStream / kChainsBefore: the run flags from the sorted keys and the
// chain tables before the accumulation; in-stream, every level's offsets too.
template <class Curve>
void MsmGpu<Curve>::early_chain_tables(const Shape& s, const Buffers& b, size_t e0, size_t ecount) {
  hipLaunchKernelGGL(chain_flags_kernel, dim3(grid_for(s.T)), dim3(kBlock), 0, stream_, b.ents2, s.key_c,
                     (uint64_t)e0, (uint64_t)(e0 + ecount), s.K, (uint32_t)s.T, b.cflags, b.clast);
  TA_HIP(hipGetLastError());
  build_chains(s, b);
  if (s.chain_mode == kChainsInStream) {
    hipLaunchKernelGGL(join_offsets_all_kernel, dim3(1), dim3(kJoinOffBlock), 0, stream_, b.cbeg, b.cend, b.dscal,
                       s.K2, (uint32_t)s.T, s.lv_max, (size_t)s.T + 2, b.early_ltab);
    TA_HIP(hipGetLastError());
  }
  TA_HIP(hipEventRecord(ev_[kMarkChainsRead], stream_));  // chain count and longest chain read back
}

// ent_mode: the entry reads of the limb-field accumulations (seg_acc_limb_body's
// kEnt): 2 LDS-staged chunks, 1 16-byte pairs, 0 8-byte loads.
template <class Curve>
typename MsmGpu<Curve>::AccLaunch MsmGpu<Curve>::acc_launch(bool raw, int ent_mode) const {
  const AccFields& f = acc_;
  AccLaunch a{nullptr, 1, 0};
  if constexpr (std::is_same_v<Curve, Bn254G1>) {
    // 29-bit-limb accumulation (BN254 G1 default; set_variant bits 13 / 17: base prefetch A/B:
    // the next base 0 not prefetched, 1 in registers, 2 via LDS-DMA)
    const int prefetch = (variant_ & 131072) ? 2 : (variant_ & 8192) ? 1 : 0;
    if (f.acc29) a.sched |= kSchedAcc29;
    if (f.acc29 && prefetch == 0 && ent_mode == 2) a.sched |= kSchedEntStaged;
    using Acc29K = decltype(&seg_acc29_kernel<0, true, 0>);
    const Acc29K k0 = ent_mode == 2 ? (raw ? seg_acc29_kernel<0, true, 2> : seg_acc29_kernel<0, false, 2>)
                      : ent_mode == 1 ? (raw ? seg_acc29_kernel<0, true, 1> : seg_acc29_kernel<0, false, 1>)
                                      : (raw ? seg_acc29_kernel<0, true, 0> : seg_acc29_kernel<0, false, 0>);
    if (f.acc29)
      a.kernel = prefetch == 2   ? (raw ? seg_acc29_kernel<2, true, 0> : seg_acc29_kernel<2, false, 0>)
                 : prefetch == 1 ? (raw ? seg_acc29_kernel<1, true, 0> : seg_acc29_kernel<1, false, 0>)
                                 : k0;
  } else if constexpr (std::is_same_v<Curve, Bls381G1>) {
    if (f.acc28) {
      a.sched |= kSchedAcc28;
      if (ent_mode == 2) a.sched |= kSchedEntStaged;
      a.kernel = raw ? (ent_mode == 2 ? seg_acc28_kernel<2, true> : ent_mode == 1 ? seg_acc28_kernel<1, true>
                                                                                  : seg_acc28_kernel<0, true>)
                     : (ent_mode == 2 ? seg_acc28_kernel<2, false> : ent_mode == 1 ? seg_acc28_kernel<1, false>
                                                                                   : seg_acc28_kernel<0, false>);
    }
  } else {
    // G2: a lane pair per virtual thread (set_variant bit 15, A/B; bit 16: inline 12-limb products)
    constexpr bool kCallDefault = Curve::F::Base::N == 12;
    const bool pair_inline = !(variant_ & 65536);
    auto* pair_kernel = pair_inline ? &seg_acc_pair_kernel<Curve, false> : &seg_acc_pair_kernel<Curve, kCallDefault>;
    // (kCallDefault is false for 8-limb fields: both entries are the inline kernel there)
    if (f.pair_acc) {
      a.sched |= kSchedLanePair;
      a.lanes = 2;
    }
    // the limb-field pairs (BLS12-381: 28-bit, BN254: 29-bit; bit 20 restores the FIPS pair)
    using LimbPol = std::conditional_t<std::is_same_v<Curve, Bls381G2>, PairPol28, PairPol29>;
    if (f.pair_acc && f.pair_limb) {
      a.sched |= std::is_same_v<Curve, Bls381G2> ? kSchedAcc28 : kSchedAcc29;
      // staged entries for BLS12-381 (2^24 accumulation 88.7 -> 88.0 ms); BN254 G2
      // measured 12.21 -> 12.32 ms at 2^22 with them (profiles/r06i/ab_entries_staged.log)
      const bool staged = ent_mode == 2 && std::is_same_v<Curve, Bls381G2>;
      if (staged) a.sched |= kSchedEntStaged;
      a.kernel = staged ? (raw ? &seg_acc_pair_limb_kernel<LimbPol, true, true>
                               : &seg_acc_pair_limb_kernel<LimbPol, true, false>)
                        : (raw ? &seg_acc_pair_limb_kernel<LimbPol, false, true>
                               : &seg_acc_pair_limb_kernel<LimbPol, false, false>);
    } else if (f.pair_acc) {
      a.kernel = pair_kernel;
    }
  }
  if (!a.kernel) a.kernel = &seg_acc_kernel<Curve>;  // the one-lane FIPS accumulation
  return a;
}

template <class Curve>
void MsmGpu<Curve>::accumulate(const Shape& s, const Buffers& b, const Aff* d_bases, unsigned g, size_t e0,
                               size_t ecount, size_t tbase) {
  const size_t Tg = (ecount + s.K - 1) / s.K;
  if (profile_) TA_HIP(hipEventRecord(gev_acc0_[g], stream_));
  // LDS-staged entry chunks when every lane's first entry is 16-byte
  // aligned, else 16-byte pairs; set_variant bit 25: the 8-byte loads (A/B)
  const int ent_mode = (variant_ & (1u << 25)) ? 0 : (s.K % 2 == 0 && e0 % 2 == 0) ? 2 : 1;
  const AccLaunch a = acc_launch(s.sb.raw, ent_mode);
  last_schedule_ |= a.sched;
  hipLaunchKernelGGL(a.kernel, dim3(grid_for(a.lanes * Tg)), dim3(kBlock), 0, stream_, d_bases, b.ents2, s.key_c,
                     (uint64_t)e0, (uint64_t)(e0 + ecount), (uint64_t)tbase, s.K, ~kSignBit, b.bucket_sum, b.pieces,
                     b.tflags, b.tlast);
  TA_HIP(hipGetLastError());
  if (profile_) TA_HIP(hipEventRecord(gev_acc1_[g], stream_));
}

// FIPS, Limb28Arith, LimbPairArith<LimbPol> or the 29-bit kernels: the limb
// fields go with the limb-field accumulation (set_variant bit 22: the FIPS
// reductions; bit 18 restores the FIPS field for BN254 G1's accumulation and
// reductions both); G2: the lane-pair reductions with the lane-pair
// accumulation (bit 15 restores both).
template <class Curve>
typename MsmGpu<Curve>::ReduceKernels MsmGpu<Curve>::reduce_kernels(bool raw) const {
  constexpr bool kG2 = std::is_same_v<Curve, Bn254G2> || std::is_same_v<Curve, Bls381G2>;
  using LimbPol = std::conditional_t<std::is_same_v<Curve, Bls381G2>, PairPol28, PairPol29>;  // G2
  const AccFields& f = acc_;
  const bool pair_limb = f.pair_acc && f.pair_limb && !(variant_ & (1 << 22));  // G2: the limb-field pair additions
  const bool limb28 = f.acc28 && !(variant_ & (1 << 22));  // BLS12-381 G1: the 28-bit reductions
  ReduceKernels k{};
  k.lanes = kG2 && f.pair_acc ? 2 : 1;
  // the join levels, the segment sums and their tree
  typename ReduceKernels::Level seg_reduce = &seg_reduce_kernel<Curve>;
  k.win_segment = &window_segment_kernel<Curve>;
  k.win_reduce = &reduce_uniform_kernel<Curve>;
  if constexpr (kG2) {
    using Limb = LimbPairArith<LimbPol>;
    using Fips = FipsPairArith<Curve>;
    if (pair_limb) {
      seg_reduce = raw ? &seg_reduce_pair_kernel<Curve, LimbPairArith<LimbPol, true, true>>
                       : &seg_reduce_pair_kernel<Curve, Limb>;
      k.win_segment = raw ? &window_segment_pair_kernel<Curve, LimbPairArith<LimbPol, true, false>>
                          : &window_segment_pair_kernel<Curve, Limb>;
      k.win_reduce = &reduce_uniform_pair_kernel<Curve, Limb>;
      k.rsum_pass1 = &window_rsum_pair_kernel<Curve, Limb>;
      k.rsum_pass2 = &window_rsum_total_pair_kernel<Curve, Limb>;
      k.rsum_fix = &window_rsum_fix_pair_kernel<Curve, Limb>;
    } else if (f.pair_acc) {
      seg_reduce = &seg_reduce_pair_kernel<Curve>;
      k.win_segment = &window_segment_pair_kernel<Curve>;
      k.win_reduce = &reduce_uniform_pair_kernel<Curve>;
      k.rsum_pass1 = &window_rsum_pair_kernel<Curve, Fips>;
      k.rsum_pass2 = &window_rsum_total_pair_kernel<Curve, Fips>;
      k.rsum_fix = &window_rsum_fix_pair_kernel<Curve, Fips>;
    }
  }
  if constexpr (std::is_same_v<Curve, Bls381G1>) {
    if (limb28) {
      seg_reduce = raw ? &seg_reduce_kernel<Curve, Limb28ArithT<true, true>> : &seg_reduce_kernel<Curve, Limb28Arith>;
      k.win_segment = raw ? &window_segment_kernel<Curve, Limb28ArithT<true, false>>
                          : &window_segment_kernel<Curve, Limb28Arith>;
      k.win_reduce = &reduce_uniform_kernel<Curve, Limb28Arith>;
    }
  }
  k.level[0][0] = k.level[0][1] = k.level[1][0] = k.level[1][1] = seg_reduce;
  if constexpr (std::is_same_v<Curve, Bn254G1>) {
    // the 29-bit reductions with the 29-bit accumulation (bit 18 restores the FIPS field for both; the window
    // sums' 29-bit kernels take both window widths and are launched by window_sums29)
    if (f.acc29) k.level[0][0] = k.level[0][1] = k.level[1][0] = k.level[1][1] = &seg_reduce29_kernel<false, false>;
    if (raw) {  // Raw pieces into level 0, Raw bucket sums out of the last level
      k.level[1][1] = &seg_reduce29_kernel<true, true>;
      k.level[1][0] = &seg_reduce29_kernel<true, false>;
      k.level[0][1] = &seg_reduce29_kernel<false, true>;
    }
  }
  // the two-level window sums (bit 23): not with the 29-bit reductions
  if constexpr (kG2) {
    if (pair_limb) {
      k.seg1 = &window_seg1_pair_kernel<Curve, LimbPairArith<LimbPol>>;
      k.seg2 = &window_seg2_pair_kernel<Curve, LimbPairArith<LimbPol>>;
      k.comb = &window_combine_pair_kernel<Curve, LimbPairArith<LimbPol>>;
    } else if (f.pair_acc) {
      k.seg1 = &window_seg1_pair_kernel<Curve, FipsPairArith<Curve>>;
      k.seg2 = &window_seg2_pair_kernel<Curve, FipsPairArith<Curve>>;
      k.comb = &window_combine_pair_kernel<Curve, FipsPairArith<Curve>>;
    }
  } else {
    bool fips = true;
    if constexpr (std::is_same_v<Curve, Bn254G1>) fips = !f.acc29;
    if constexpr (std::is_same_v<Curve, Bls381G1>) {
      if (limb28) {
        k.seg1 = &window_seg1_kernel<Curve, Limb28Arith>;
        k.seg2 = &window_seg2_kernel<Curve, Limb28Arith>;
        k.comb = &window_combine_kernel<Curve, Limb28Arith>;
        fips = false;
      }
    }
    if (fips) {
      k.seg1 = &window_seg1_kernel<Curve, FipsArith<Curve>>;
      k.seg2 = &window_seg2_kernel<Curve, FipsArith<Curve>>;
      k.comb = &window_combine_kernel<Curve, FipsArith<Curve>>;
    }
  }
  return k;
}

// Debug check (set_variant bit 21): pre-derived flags == the accumulation's
template <class Curve>
void MsmGpu<Curve>::check_early_flags(const Shape& s, const Buffers& b) {
  uint32_t* mism = static_cast<uint32_t*>(check_.ensure(sizeof(uint32_t)));
  TA_HIP(hipMemsetAsync(mism, 0, sizeof(uint32_t), stream_));
  hipLaunchKernelGGL(chain_flags_check_kernel, dim3(grid_for(s.T)), dim3(kBlock), 0, stream_, b.tflags, b.tlast,
                     b.cflags, b.clast, (uint32_t)s.T, mism);
  TA_HIP(hipGetLastError());
  uint32_t h = 0;
  TA_HIP(hipMemcpyAsync(&h, mism, sizeof(h), hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
  if (h) throw std::runtime_error("tachyon_mi355x: chain flags derived before the accumulation differ from its own");
  last_schedule_ |= kSchedChainsChecked;
}

// Every join level's output offsets when they were not built in-stream (level
// l's table: segment s of level l + 1 = [off_l[s], off_l[s + 1])), one table
// per level at ltab + l * stride.
template <class Curve>
void MsmGpu<Curve>::join_offsets(const Shape& s, const Buffers& b, uint32_t nchains, unsigned K2, unsigned levels,
                                 uint32_t* ltab, size_t stride) {
  const bool small = nchains <= kJoinSmallChains;  // offsets in one workgroup
  size_t scan2_bytes = 0;
  void* scan_tmp = nullptr;
  if (!small) {
    TA_HIP(rocprim::exclusive_scan(nullptr, scan2_bytes, b.lcnt, ltab, 0u, (size_t)nchains + 1,
                                   rocprim::plus<uint32_t>(), stream_));
    scan_tmp = scan_tmp_.ensure(scan2_bytes);
  }
  for (unsigned l = 0; l < levels; ++l) {
    uint32_t* loff = ltab + l * stride;
    const uint32_t* pbeg = l == 0 ? b.cbeg : ltab + (l - 1) * stride;
    const uint32_t* pend = l == 0 ? b.cend : pbeg + 1;
    if (small) {
      hipLaunchKernelGGL(join_offsets_kernel, dim3(1), dim3(kJoinOffBlock), 0, stream_, pbeg,
                         l == 0 ? pend : nullptr, nchains, K2, loff);
    } else {
      if (l > 0 || K2 != s.K2)  // (level 0's counts came with the read-back, for the plan's K2)
        hipLaunchKernelGGL(seg_count_kernel, dim3(grid_for((size_t)nchains + 1)), dim3(kBlock), 0, stream_, pbeg,
                           pend, nullptr, nchains, K2, b.lcnt, nullptr);
      TA_HIP(rocprim::exclusive_scan(scan_tmp, scan2_bytes, b.lcnt, loff, 0u, (size_t)nchains + 1,
                                     rocprim::plus<uint32_t>(), stream_));
    }
  }
  TA_HIP(hipGetLastError());
}

// Join buckets that cross thread boundaries (the chain count and the longest
// chain decide the levels: read back while the accumulation runs when the
// chain tables were built early).
template <class Curve>
void MsmGpu<Curve>::join(const Shape& s, const Buffers& b, const ReduceKernels& rk) {
  const size_t T = s.T;
  if (s.chain_mode != kChainsAfter) {
    if (variant_ & (1 << 21)) check_early_flags(s, b);
    TA_HIP(hipEventSynchronize(ev_[kMarkChainsRead]));
  } else {
    build_chains(s, b);
    TA_HIP(hipStreamSynchronize(stream_));
  }
  const uint32_t nchains = h_max_[0], max_len = h_max_[1];
  const unsigned K2 = join_fan_in(max_len, s.K2, T);
  const unsigned levels = join_levels(max_len, K2);
  last_levels_ = levels;
  if (nchains == 0 || levels == 0) return;
  // phase 1: every level's output offsets -- already on the device for the
  // small MSMs (join_offsets_all_kernel)
  const bool in_stream = s.chain_mode == kChainsInStream;
  if (in_stream && levels > s.lv_max) throw std::runtime_error("tachyon_mi355x: MSM join levels exceed their bound");
  const size_t stride = in_stream ? T + 2 : (size_t)nchains + 2;
  uint32_t* ltab = in_stream ? b.early_ltab : static_cast<uint32_t*>(lofs_.ensure(levels * stride * 4));
  if (!in_stream) join_offsets(s, b, nchains, K2, levels, ltab, stride);
  // phase 2: the levels, back to back on the MSM stream
  const Point* cur = b.pieces;
  size_t cur_items = 2 * T;
  Point* dst_bufs[2] = {b.lvl_buf, b.pieces};  // pieces is free once level 0 has read it
  for (unsigned l = 0; l < levels; ++l) {
    const bool last = (l + 1 == levels);
    const uint32_t* loff = ltab + l * stride;
    const uint32_t* cur_beg = l == 0 ? b.cbeg : ltab + (l - 1) * stride;
    const uint32_t* cur_end = l == 0 ? b.cend : cur_beg + 1;
    size_t out_items = cur_items / K2 + nchains + 1;
    Point* dst = dst_bufs[l & 1];
    hipLaunchKernelGGL(rk.level[l == 0][last], dim3(grid_for(rk.lanes * out_items)), dim3(kBlock), 0, stream_, cur,
                       cur_beg, cur_end, loff, nchains, K2, dst, last ? b.cbucket : nullptr, b.bucket_sum);
    TA_HIP(hipGetLastError());
    cur = dst;
    cur_items = out_items;
  }
}

// Two-level window sums (window_seg1/2 + combine) under set_variant bit 23,
// for the G2 lane pairs and the one-lane BLS12-381 G1 / FIPS reductions: an
// A/B that lost -- BLS12-381 G2 2^24 109.0 vs 106.2 ms (reduction 16.3 vs
// 13.7), BN254 G2 2^20 6.6 vs 5.15 ms (2.18 vs 0.95), Groth16 2^20 12.8 vs
// 11.4 ms (profiles/r05w/): the extra launches of two binary trees over
// W x B/16 and W x B/1024 partial sums cost more than the fix-ups they save.
// The one-level kernels (per-segment (jL) R fix-up) stay the default.
template <class Curve>
void MsmGpu<Curve>::window_sums_two_level(const Shape& s, const Buffers& b, const ReduceKernels& rk,
                                          Point* d_windows) {
  const unsigned W = s.W, B = s.B, lanes = rk.lanes;
  const unsigned L1 = std::min(16u, B), S1 = B / L1;
  const unsigned L2 = std::min(64u, S1), S2 = S1 / L2;
  // A_j, R_j (W S1 each), level-2 sums (W S2), two tree ping-pong halves, the two window sums
  const size_t tmp = (size_t)W * ((S1 + 1) / 2 + 1);
  Point* segA = static_cast<Point*>(
      seg_a_.ensure(((size_t)2 * W * S1 + (size_t)W * S2 + 2 * tmp + 2 * W) * sizeof(Point)));
  Point* segR = segA + (size_t)W * S1;
  Point* seg2o = segR + (size_t)W * S1;
  Point* tA = seg2o + (size_t)W * S2;
  Point* tB = tA + tmp;
  Point* winA = tB + tmp;
  Point* winB = winA + W;
  hipLaunchKernelGGL(rk.seg1, dim3(grid_for(lanes * (size_t)W * S1)), dim3(kBlock), 0, stream_, b.bucket_sum, W, B, L1,
                     segA, segR);
  hipLaunchKernelGGL(rk.seg2, dim3(grid_for(lanes * (size_t)W * S2)), dim3(kBlock), 0, stream_, segR, W, S1, L2, seg2o);
  TA_HIP(hipGetLastError());
  // binary trees (win_reduce) of the W x S arrays down to one point per window
  auto tree = [&](Point* src, unsigned S, Point* dst) {
    Point* cur = src;
    Point* bufs[2] = {tA, tB};
    int k = 0;
    while (S > 1) {
      const unsigned S_out = (S + 1) / 2;
      Point* o = (S_out == 1) ? dst : bufs[k];
      hipLaunchKernelGGL(rk.win_reduce, dim3(grid_for(lanes * (size_t)W * S_out)), dim3(kBlock), 0, stream_, cur, W, S,
                         2u, o);
      TA_HIP(hipGetLastError());
      cur = o;
      k ^= 1;
      S = S_out;
    }
    if (cur != dst) TA_HIP(hipMemcpyAsync(dst, cur, W * sizeof(Point), hipMemcpyDeviceToDevice, stream_));
  };
  tree(segA, S1, winA);
  tree(seg2o, S2, winB);
  hipLaunchKernelGGL(rk.comb, dim3(grid_for(lanes * (size_t)W)), dim3(kBlock), 0, stream_, winA, winB, W, L1, d_windows);
  TA_HIP(hipGetLastError());
}

// set_variant bit 12: segments of L buckets, workgroup trees of kWinBlock nodes, launches until one node per window
template <class Curve>
void MsmGpu<Curve>::window_sums_by_trees(const Shape& s, const Buffers& b, Point* d_windows) {
  const unsigned W = s.W, B = s.B;
  unsigned L = s.seg_tree, log_l = 0;
  while ((1u << log_l) < L) ++log_l;
  unsigned units = B / L;
  unsigned groups = (units + kWinBlock - 1) / kWinBlock;
  const size_t lds = (size_t)kWinBlock * sizeof(Point);  // kWinBlock / 2 (V, Rs) pairs
  Point* na = static_cast<Point*>(seg_a_.ensure((size_t)W * groups * 2 * sizeof(Point)));
  Point* nb_ = static_cast<Point*>(seg_b_.ensure((size_t)W * ((groups + kWinBlock - 1) / kWinBlock) * 2 * sizeof(Point)));
  hipLaunchKernelGGL((window_tree_kernel<Curve, true>), dim3(groups, W), dim3(kWinBlock), lds, stream_, b.bucket_sum, B,
                     L, log_l, nullptr, units, na);
  TA_HIP(hipGetLastError());
  Point* cur_n = na;
  Point* nxt_n = nb_;
  while (groups > 1) {
    units = groups;
    groups = (units + kWinBlock - 1) / kWinBlock;
    hipLaunchKernelGGL((window_tree_kernel<Curve, false>), dim3(groups, W), dim3(kWinBlock), lds, stream_, nullptr,
                       B, L, log_l, cur_n, units, nxt_n);
    TA_HIP(hipGetLastError());
    std::swap(cur_n, nxt_n);
  }
  // the root V of every window: node pairs (V, Rs), stride 2
  TA_HIP(hipMemcpy2DAsync(d_windows, sizeof(Point), cur_n, 2 * sizeof(Point), sizeof(Point), W,
                          hipMemcpyDeviceToDevice, stream_));
}

// The default: per-segment running sums (one pass, or the two-pass sums of
// the G2 lane pairs under set_variant bit 24), then a binary tree over them.
template <class Curve>
void MsmGpu<Curve>::window_sums_by_segments(const Shape& s, const Buffers& b, const ReduceKernels& rk,
                                            Point* d_windows) {
  const unsigned W = s.W, B = s.B, lanes = rk.lanes;
  unsigned S = B / s.seg;
  Point* seg_a = static_cast<Point*>(seg_a_.ensure((size_t)W * S * sizeof(Point)));
  Point* seg_b = static_cast<Point*>(seg_b_.ensure((size_t)W * S * sizeof(Point)));
  if (rk.rsum_pass1 && (variant_ & (1 << 24))) {  // the two-pass segment sums (G2 lane pairs, A/B)
    Point* rs = static_cast<Point*>(rsum_.ensure((size_t)W * B * sizeof(Point)));
    hipLaunchKernelGGL(rk.rsum_pass1, dim3(grid_for(lanes * (size_t)W * S)), dim3(kBlock), 0, stream_, b.bucket_sum, W,
                       B, s.seg, rs);
    hipLaunchKernelGGL(rk.rsum_pass2, dim3(grid_for(lanes * (size_t)W * S)), dim3(kBlock), 0, stream_, rs, W, B, s.seg,
                       seg_a);
    hipLaunchKernelGGL(rk.rsum_fix, dim3(grid_for(lanes * (size_t)W * S)), dim3(kBlock), 0, stream_, rs, W, B, s.seg,
                       seg_a);
  } else {
    hipLaunchKernelGGL(rk.win_segment, dim3(grid_for(lanes * (size_t)W * S)), dim3(kBlock), 0, stream_, b.bucket_sum, W,
                       B, s.seg, seg_a);
  }
  TA_HIP(hipGetLastError());
  Point* s_cur = seg_a;
  Point* s_nxt = seg_b;
  // binary tree over the segment sums: these levels run a few hundred waves,
  // so they are latency-bound and the sequential adds per thread set the time
  // (fan-in 16 -> 2 saved ~0.4 ms at 2^21..2^23)
  constexpr unsigned KW = 2;
  while (S > 1) {
    unsigned S_out = (S + KW - 1) / KW;
    Point* dst = (S_out == 1) ? d_windows : s_nxt;
    hipLaunchKernelGGL(rk.win_reduce, dim3(grid_for(lanes * (size_t)W * S_out)), dim3(kBlock), 0, stream_, s_cur, W, S,
                       KW, dst);
    TA_HIP(hipGetLastError());
    std::swap(s_cur, s_nxt);
    S = S_out;
  }
  if (B / s.seg == 1) {
    TA_HIP(hipMemcpyAsync(d_windows, seg_a, W * sizeof(Point), hipMemcpyDeviceToDevice, stream_));
  }
}

// BN254 G1 over the 29-bit field: the window sums of both width classes in the
// same launches (pass29 says which windows go by the scan and which by
// segments of one length L): one segment pass, the binary levels until the
// widest window has <= kBlock sums left, one tree launch for the rest.
template <class Curve>
void MsmGpu<Curve>::window_sums29(const Shape& s, const Buffers& b, Point* d_windows) {
  if constexpr (std::is_same_v<Curve, Bn254G1>) {
    const bool raw = s.sb.raw;
    const Pass29 p = pass29(s.mixed ? s.narrow : s.W, s.W, s.B, s.seg, raw);
    auto buckets_of = [&](unsigned w) {  // window w's first bucket: w, and the wide windows below it once more, times B
      const unsigned units = w + (s.mixed && w > s.narrow ? w - s.narrow : 0u);
      return reinterpret_cast<Point*>(reinterpret_cast<char*>(b.bucket_sum) + (size_t)units * s.B * s.sb.slot);
    };
    auto* scan = raw ? &window_scan29_kernel<true> : &window_scan29_kernel<false>;
    if (p.scan_lo) {
      hipLaunchKernelGGL(scan, dim3(p.scan_lo), dim3(kBlock), 0, stream_, b.bucket_sum, s.B, d_windows);
      TA_HIP(hipGetLastError());
    }
    if (p.scan_hi) {
      hipLaunchKernelGGL(scan, dim3(p.scan_hi), dim3(kBlock), 0, stream_, buckets_of(p.scan_lo), 2 * s.B,
                         d_windows + p.scan_lo);
      TA_HIP(hipGetLastError());
    }
    if (p.W == 0) return;
    // the segment pass: windows [first, first + W), `narrow` of them with B buckets, the others with 2 B
    Point* out = d_windows + p.first;
    unsigned S = s.B / p.L;
    const unsigned wide = p.W - p.narrow;
    Point* s_cur = static_cast<Point*>(seg_a_.ensure(p.sums * sizeof(Point)));
    Point* s_nxt = static_cast<Point*>(seg_b_.ensure(p.sums * sizeof(Point)));
    auto* segment = raw ? &window_segment29_kernel<true> : &window_segment29_kernel<false>;
    hipLaunchKernelGGL(segment, dim3(grid_for(p.sums)), dim3(kBlock), 0, stream_, buckets_of(p.first), p.W, p.narrow, s.B,
                       p.L, s_cur);
    TA_HIP(hipGetLastError());
    // (these levels run a few hundred waves, latency-bound: fan-in 2, see window_sums_by_segments)
    while ((wide ? 2 * S : S) > kBlock) {
      if (wide && (S & 1)) throw std::runtime_error("tachyon_mi355x: odd segment count under windows of two widths");
      hipLaunchKernelGGL(reduce_uniform29_kernel, dim3(grid_for((size_t)p.narrow * ((S + 1) / 2) + (size_t)wide * S)),
                         dim3(kBlock), 0, stream_, s_cur, p.W, p.narrow, S, 2u, s_nxt);
      TA_HIP(hipGetLastError());
      std::swap(s_cur, s_nxt);
      S = (S + 1) / 2;
    }
    hipLaunchKernelGGL(window_tree29_kernel, dim3(p.W), dim3(kBlock), 0, stream_, s_cur, p.narrow, S, out);
    TA_HIP(hipGetLastError());
  }
}

// Mixed widths (all but BN254 G1's 29-bit field, window_sums29): one pass per
// width class over the class's contiguous buckets -- B is uniform inside a
// class, so the kernels are the uniform ones, each class with the segment
// lengths of its own window and bucket counts.
template <class Curve>
void MsmGpu<Curve>::window_sums(const Shape& s, const Buffers& b, const ReduceKernels& rk, Point* d_windows) {
  if (sums_by_pass29(acc_)) {
    if (!s.mixed && (variant_ & (1u << 19)) && !window_sums_by_scan(acc_, s.B) && s.B / s.seg <= kBlock) {
      if constexpr (std::is_same_v<Curve, Bn254G1>) {
        auto* segtree = s.sb.raw ? &window_segtree29_kernel<true> : &window_segtree29_kernel<false>;
        hipLaunchKernelGGL(segtree, dim3(s.W), dim3(kBlock), 0, stream_, b.bucket_sum, s.B, s.seg, d_windows);
        TA_HIP(hipGetLastError());
      }
      return;
    }
    return window_sums29(s, b, d_windows);
  }
  if (s.mixed) {
    const unsigned classes[2][3] = {{0, s.narrow, s.B}, {s.narrow, s.W - s.narrow, 2 * s.B}};  // first window, windows, B
    // the segment sums of both classes share seg_a_ / seg_b_: sized for the larger
    // before either is enqueued (none where both classes go by the scan)
    if (const size_t seg_sums = mixed_seg_sums(acc_, s.narrow, s.W, s.B)) {
      seg_a_.ensure(seg_sums * sizeof(Point));
      seg_b_.ensure(seg_sums * sizeof(Point));
    }
    for (const auto& cl : classes) {
      if (cl[1] == 0) continue;
      Shape sc = s;
      Buffers bc = b;
      sc.mixed = false;
      sc.W = cl[1], sc.B = cl[2];
      sc.seg = class_seg(cl[1], cl[2]);
      sc.seg_tree = MsmPlan::seg_tree_for(cl[1], cl[2]);
      bc.bucket_sum = reinterpret_cast<Point*>(reinterpret_cast<char*>(b.bucket_sum) +
                                               (size_t)cl[0] * s.B * s.sb.slot);
      window_sums(sc, bc, rk, d_windows + cl[0]);
    }
    return;
  }
  if (rk.seg1 && (variant_ & (1 << 23)) && !acc_.tree_reduce) return window_sums_two_level(s, b, rk, d_windows);
  if (acc_.tree_reduce) return window_sums_by_trees(s, b, d_windows);
  window_sums_by_segments(s, b, rk, d_windows);
}

template <class Curve>
void MsmGpu<Curve>::enqueue(const Aff* d_bases, const Fr* d_scalars, size_t n, const MsmPlan& plan,
                            Point* d_windows) {
  const Shape s = make_shape(n, plan);
  const Buffers b = carve(s);
  const ReduceKernels rk = reduce_kernels(s.sb.raw);
  last_schedule_ = (s.ss.fused ? kSchedFusedRecode : 0u) | (s.ss.own_sort ? kSchedRecodeFedSort : 0u) |
                   (s.ss.fused && s.ss.narrow ? kSchedNarrowStaging : 0u) | (s.mixed ? kSchedMixedWindows : 0u);
  if (profile_) TA_HIP(hipEventRecord(ev_[kMarkUploaded], stream_));
  uint32_t* digit_off = recode(s, b, d_scalars);
  TA_HIP(hipEventRecord(ev_[kMarkRecoded], stream_));  // recode done (also the profile mark)
  if (b.sort_stream != stream_) TA_HIP(hipStreamWaitEvent(b.sort_stream, ev_[kMarkRecoded], 0));
  // per group: radix sort of its (window, bucket, point) entries, then accumulation
  size_t tbase = 0;
  acc_launches_ = s.ngroups;
  for (unsigned g = 0; g < s.ngroups; ++g) {
    const unsigned w0 = g * s.G, w1 = std::min(s.W, w0 + s.G);
    const size_t e0 = (size_t)w0 * s.epw, ecount = (size_t)(w1 - w0) * s.epw;
    sort_group(s, b, g, e0, ecount, digit_off);
    if (g == 0 && pending_host_bases_) upload_pending_bases(d_bases, n);
    if (s.chain_mode != kChainsAfter) early_chain_tables(s, b, e0, ecount);
    accumulate(s, b, d_bases, g, e0, ecount, tbase);
    tbase += (ecount + s.K - 1) / s.K;
  }
  if (profile_) TA_HIP(hipEventRecord(ev_[kMarkAccumulated], stream_));  // last accumulation done
  join(s, b, rk);
  window_sums(s, b, rk, d_windows);
  if (profile_) TA_HIP(hipEventRecord(ev_[kMarkEnd], stream_));
}

template <class Curve>
void MsmGpu<Curve>::run_windows(const void* bases, const void* scalars, size_t n, std::vector<Point>* out,
                                MsmPlan* plan_out) {
  MsmPlan plan = run_plan(n, force_c_);
  if (mixed_w_ && !plan.mixed)  // asked for both: an error, not a silent uniform run
    throw std::runtime_error("tachyon_mi355x: mixed-width MSM windows are set: no window range, batch, fold, forced "
                             "window bits or window groups with them");
  // what the variant bits select (sort_knobs, acc_fields), decoded once per run
  sort_ = sort_knobs(variant_);
  acc_ = acc_fields(variant_);
  sort_cfg_ = (variant_ >> 4) & 3;  // bits 4-5: onesweep tile shape
#ifdef TACHYON_TUNING_KNOBS
  if (const char* e = getenv("TACHYON_ONESWEEP_CFG")) sort_cfg_ = (unsigned)std::clamp(atoi(e), 0, 5);
#endif
  if (plan_out) *plan_out = plan;
  if (fold_ > 1 && (plan.w_begin != 0 || plan.w_end != plan.windows || plan.windows % fold_ != 0))
    throw std::runtime_error("tachyon_mi355x: an MSM fold must divide the plan's window count (all windows)");
  // window sums (per MSM of a batch, run_batch; W / fold of a folded run)
  const unsigned nwin = (fold_ > 1 ? plan.windows / fold_ : plan.active()) * batch_;
  out->assign(nwin, Point::zero());
  if (n == 0 || plan.active() == 0) return;
  if (profile_) TA_HIP(hipEventRecord(ev_[kMarkStart], stream_));
  const Aff* d_bases = static_cast<const Aff*>(bases);
  const Fr* d_scalars = static_cast<const Fr*>(scalars);
  pending_host_bases_ = nullptr;
  if (!is_device_pointer(bases)) {  // uploaded inside enqueue(), overlapping the recode and the sort
    d_bases = static_cast<const Aff*>(bases_.ensure(n * sizeof(Aff)));
    pending_host_bases_ = bases;
  }
  if (!is_device_pointer(scalars)) {
    void* p = scalars_.ensure(n * sizeof(Fr));
    TA_HIP(hipMemcpyAsync(p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    d_scalars = static_cast<const Fr*>(p);
  }
  Point* d_windows = static_cast<Point*>(windows_.ensure(std::max(1u, nwin) * sizeof(Point)));
  enqueue(d_bases, d_scalars, n, plan, d_windows);
  TA_HIP(hipMemcpyAsync(out->data(), d_windows, nwin * sizeof(Point), hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
  for (auto& p : *out) p = p.canonical();  // device values live in [0, 2p)
  if (profile_) {
    TA_HIP(hipEventElapsedTime(&timings_.h2d, ev_[kMarkStart], ev_[kMarkUploaded]));
    TA_HIP(hipEventElapsedTime(&timings_.recode, ev_[kMarkUploaded], ev_[kMarkRecoded]));
    TA_HIP(hipEventElapsedTime(&timings_.sort, ev_[kMarkRecoded], ev_[kMarkSorted]));
    // sort: recode end -> last sort end; prep: recode end -> last accumulation end
    // (sort and accumulation overlap); acc: sum of the accumulation launches
    TA_HIP(hipEventElapsedTime(&timings_.prep, ev_[kMarkRecoded], ev_[kMarkAccumulated]));
    timings_.acc = 0;
    for (unsigned g = 0; g < acc_launches_; ++g) {
      float ms = 0;
      TA_HIP(hipEventElapsedTime(&ms, gev_acc0_[g], gev_acc1_[g]));
      timings_.acc += ms;
    }
    timings_.acc_launches = (float)acc_launches_;
    TA_HIP(hipEventElapsedTime(&timings_.reduce, ev_[kMarkAccumulated], ev_[kMarkEnd]));
    TA_HIP(hipEventElapsedTime(&timings_.total, ev_[kMarkStart], ev_[kMarkEnd]));
  }
}

}  // namespace tachyon_amd::msm

#include "msm_ceiling.h"

namespace tachyon_amd::msm {

// Horner over windows, high to low, c doublings in between
// (PippengerBase::AccumulateWindowSums, pippenger_base.h:59-77).
template <class Curve>
typename MsmGpu<Curve>::Point MsmGpu<Curve>::combine_windows(const std::vector<Point>& ws, unsigned c) {
  Point total = Point::zero();
  for (size_t w = ws.size(); w-- > 0;) {
    if (w + 1 < ws.size())
      for (unsigned k = 0; k < c; ++k) total = total.dbl();
    total = total + ws[w];
  }
  return total;
}

// ... over a run's active windows: the doublings between two windows are the
// width of the lower one (uniform plans: c)
template <class Curve>
typename MsmGpu<Curve>::Point MsmGpu<Curve>::combine_windows(const std::vector<Point>& ws, const MsmPlan& plan) {
  if (!plan.mixed) return combine_windows(ws, plan.c);
  Point total = Point::zero();
  for (size_t w = ws.size(); w-- > 0;) {
    if (w + 1 < ws.size())
      for (unsigned k = 0; k < plan.width((unsigned)w); ++k) total = total.dbl();
    total = total + ws[w];
  }
  return total;
}

// Host-resident inputs of >= 2^24 points: the upload, not the GPU, is the
// bound (≈6.4 GB at ≈54 GB/s for 2^26 BN254 G1 against ≈95 ms of kernels),
// and the accumulation of a window needs every base, so a single MSM cannot
// start before the last byte arrives.  Split the points into chunks of
// ≥ 2^22 (the kParallelTerm decomposition, pippenger_adapter.h:82-113): a
// copy thread queues every chunk's H2D on copy_stream_ (recording one event
// per chunk) while this thread runs the MSM of chunk k as soon as its event
// is recorded, so the kernels of chunk k overlap the upload of k+1..; the
// chunk results are added on the host.  TACHYON_MSM_HOST_CHUNKS overrides
// the chunk count (1 = one MSM after one upload).  msm_benchmark_gpu sweep
// (host-resident, s): 2^26 chunks 1/4/6/8/12/16 -> 0.193/0.142/0.143/0.136/
// 0.140/0.140; 2^24 1/2/3/4/8 -> 0.053/0.046/0.043/0.042/0.043; 2^22 stays
// whole (1/3/4 -> 0.015/0.021/0.018: the per-chunk reduction dominates).
inline size_t host_chunk_count(size_t n) {
  if (const char* e = getenv("TACHYON_MSM_HOST_CHUNKS")) return std::clamp<size_t>(atoi(e), 1, 64);
  if (n < (size_t(1) << 24)) return 1;
  return std::min<size_t>(8, n >> 22);
}

template <class Curve>
typename MsmGpu<Curve>::Point MsmGpu<Curve>::run_host_pipelined(const void* bases, const void* scalars, size_t n,
                                                                size_t chunks) {
  const bool host_b = !is_device_pointer(bases), host_s = !is_device_pointer(scalars);
  Aff* d_b = host_b ? static_cast<Aff*>(bases_.ensure(n * sizeof(Aff))) : const_cast<Aff*>(static_cast<const Aff*>(bases));
  Fr* d_s = host_s ? static_cast<Fr*>(scalars_.ensure(n * sizeof(Fr))) : const_cast<Fr*>(static_cast<const Fr*>(scalars));
  if (!copy_stream_) TA_HIP(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
  while (chunk_ev_.size() < chunks) {
    hipEvent_t e;
    TA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    chunk_ev_.push_back(e);
  }
  const size_t step = (n + chunks - 1) / chunks;
  int device = 0;
  TA_HIP(hipGetDevice(&device));
  std::mutex mu;
  std::condition_variable cv;
  size_t ready = 0;  // chunks whose copies and event are queued
  bool failed = false;
  std::exception_ptr copy_error;
  std::thread copier([&] {
    try {
      TA_HIP(hipSetDevice(device));
      for (size_t k = 0; k < chunks; ++k) {
        const size_t lo = std::min(n, k * step), len = std::min(step, n - lo);
        if (host_b && len)
          TA_HIP(hipMemcpyAsync(d_b + lo, static_cast<const Aff*>(bases) + lo, len * sizeof(Aff),
                                hipMemcpyHostToDevice, copy_stream_));
        if (host_s && len)
          TA_HIP(hipMemcpyAsync(d_s + lo, static_cast<const Fr*>(scalars) + lo, len * sizeof(Fr),
                                hipMemcpyHostToDevice, copy_stream_));
        TA_HIP(hipEventRecord(chunk_ev_[k], copy_stream_));
        {
          std::lock_guard<std::mutex> lk(mu);
          ready = k + 1;
        }
        cv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      copy_error = std::current_exception();
      failed = true;
      cv.notify_all();
    }
  });
  struct Joiner {
    std::thread& t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } joiner{copier};
  Point total = Point::zero();
  std::vector<Point> ws;
  MsmPlan plan;
  for (size_t k = 0; k < chunks; ++k) {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return ready > k || failed; });
      if (failed) break;
    }
    const size_t lo = std::min(n, k * step), len = std::min(step, n - lo);
    if (!len) continue;
    TA_HIP(hipStreamWaitEvent(stream_, chunk_ev_[k], 0));
    run_windows(d_b + lo, d_s + lo, len, &ws, &plan);
    total = total + combine_windows(ws, plan);
  }
  copier.join();
  if (copy_error) std::rethrow_exception(copy_error);
  return total;
}

// BN254 G1 over the 29-bit field with at most kBlock buckets per window: the
// window sums are one scan launch per window, with no segment sums (window_sums;
// work_bytes leaves them out of the estimate)
template <class Curve>
bool MsmGpu<Curve>::window_sums_by_scan(const AccFields& f, unsigned buckets) {
  return std::is_same_v<Curve, Bn254G1> && f.acc29 && !f.tree_reduce && buckets <= detail::kBlock;
}

// Mixed widths: a width class takes the segment length of its own window and
// bucket counts (G2: twice the G1 rule's length, as run_plan's uniform rule)
template <class Curve>
unsigned MsmGpu<Curve>::class_seg(unsigned windows, unsigned buckets) {
  unsigned seg = MsmPlan::seg_for(windows, buckets);
  if constexpr (std::is_same_v<Curve, Bn254G2> || std::is_same_v<Curve, Bls381G2>)
    seg = std::min(buckets, std::min(128u, seg * 2));
  return seg;
}

template <class Curve>
bool MsmGpu<Curve>::sums_by_pass29(const AccFields& f) {
  return std::is_same_v<Curve, Bn254G1> && f.acc29 && !f.tree_reduce;
}

// Threads of window_segment29_kernel the device holds at once: the kernel's
// resident blocks per CU (as the runtime prices its registers) times the CUs.
template <class Curve>
size_t MsmGpu<Curve>::resident_threads29(bool raw) {
  static size_t cached[2] = {0, 0};  // (every device of a process is the same part)
  if constexpr (std::is_same_v<Curve, Bn254G1>) {
    if (!cached[raw]) {
      int dev = 0, cus = 0, blocks = 0;
      TA_HIP(hipGetDevice(&dev));
      TA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
      auto* segment = raw ? &window_segment29_kernel<true> : &window_segment29_kernel<false>;
      TA_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, segment, (int)kBlock, 0));
      cached[raw] = (size_t)std::max(1, blocks) * std::max(1, cus) * kBlock;
    }
  }
  return cached[raw];
}

// How window_sums29 covers `narrow` windows of B buckets and W - narrow of 2 B:
// a class with at most kBlock buckets per window goes by the scan, the other
// windows by segments of one length L.  L is `seg`, the small-MSM rule's
// (MsmPlan::seg_for); where that rule stops at its cap of 64 although the
// segment threads still need more than one resident round of the kernel, L
// doubles until they fit one (the rounds of the serial chain set the time, not
// the additions: 2^26, 15.7 M buckets: L = 128, 122,880 threads), up to
// kSeg29Max.  set_window_segment overrides it (tests, tuning).
template <class Curve>
typename MsmGpu<Curve>::Pass29 MsmGpu<Curve>::pass29(unsigned narrow, unsigned W, unsigned B, unsigned seg,
                                                     bool raw) const {
  Pass29 p{};
  p.narrow = narrow, p.W = W;
  if (B <= kBlock) {  // the narrow class by the scan (window_sums_by_scan)
    p.scan_lo = narrow, p.first = narrow, p.narrow = 0, p.W = W - narrow;
    if (2 * B <= kBlock) p.scan_hi = p.W, p.first = W, p.W = 0;
  }
  if (p.W == 0) return p;
  const size_t nb = ((size_t)p.narrow + 2 * (size_t)(p.W - p.narrow)) * B;
  if (p.narrow != W) seg = MsmPlan::seg_for(1, (unsigned)std::min<size_t>(nb, 1u << 31));  // both classes' buckets
  if (seg_force_) {
    seg = seg_force_;
  } else if (seg == 64) {
    const size_t resident = resident_threads29(raw);
    while (seg < kSeg29Max && nb / seg > resident) seg *= 2;
  }
  p.L = std::min(seg, B);
  p.sums = nb / p.L;
  return p;
}

template <class Curve>
size_t MsmGpu<Curve>::mixed_seg_sums(const AccFields& f, unsigned narrow, unsigned W, unsigned B) {
  const unsigned classes[2][2] = {{narrow, B}, {W - narrow, 2 * B}};  // windows, buckets per window
  size_t sums = 0;
  for (const auto& cl : classes)
    if (cl[0] && !window_sums_by_scan(f, cl[1])) sums = std::max(sums, (size_t)cl[0] * (cl[1] / class_seg(cl[0], cl[1])));
  return sums;
}

// The plan run_windows runs n points by: MsmPlan::make for the context's
// window range, then the variant bits that change it.
template <class Curve>
MsmPlan MsmGpu<Curve>::run_plan(size_t n, unsigned c) const {
  MsmPlan plan = MsmPlan::make(n, Fr::Config::kModulusBits, c, range_begin_, range_end_);
  // Mixed widths: for a plain run only -- all windows, one MSM, no fold, no
  // forced window bits, one sort group.  Set explicitly (set_mixed_windows),
  // any other run is an error (run_windows throws); as the size's default, the
  // other runs keep the uniform plan, and set_variant bit 27 restores it for
  // the plain run (A/B).
  const bool plain = range_begin_ == 0 && range_end_ == ~0u && batch_ == 1 && fold_ == 1 && c == 0 &&
                     (((variant_ >> 2) & 3) == 0 || ((variant_ >> 2) & 3) == 3);
  const unsigned mixed_w = mixed_w_ ? mixed_w_ : (variant_ & kMsmVariantUniformWindows) ? 0u : default_mixed_windows(n);
  if (mixed_w && plain) plan = MsmPlan::make_mixed(n, Fr::Config::kModulusBits, mixed_w);
  // G2: running-sum segments twice the G1 rule's length -- a G2 fix-up costs
  // more against the latency-bound loop (BLS12-381 G2 2^24 reduction 13.7 ->
  // 13.0 ms at L = 128, BN254 G2 2^22 1.75 -> 1.64 ms at L = 32;
  // profiles/r05am, r05an)
  if constexpr (std::is_same_v<Curve, Bn254G2> || std::is_same_v<Curve, Bls381G2>) {
#ifdef TACHYON_TUNING_KNOBS
    if (!getenv("TACHYON_MSM_SEG"))
#endif
      if (!plan.mixed) plan.seg = std::min(plan.buckets, std::min(128u, plan.seg * 2));
  }
  switch (variant_ & 3) {  // accumulation chunk experiments
    case 1: plan.K = std::min(2048u, plan.K * 2); break;
    case 2: plan.K = std::min(2048u, plan.K * 4); break;
    case 3: plan.K = std::max(4u, plan.K / 2); break;
    default: break;
  }
  switch ((variant_ >> 2) & 3) {  // windows per sort/accumulate group
    case 1: plan.group = 1; break;
    case 2: plan.group = 2; break;
    case 3: plan.group = plan.active(); break;
    default: break;
  }
  return plan;
}

template <class Curve>
typename MsmGpu<Curve>::SortKnobs MsmGpu<Curve>::sort_knobs(int variant) {
  SortKnobs k;
  k.fuse_recode = !(variant & 128);  // bit 7: the separate recode + full sort (A/B)
  static constexpr uint32_t kSpt[] = {detail::kRecodeSpt, 1, 4, 3};
  k.spt = kSpt[(variant >> 8) & 3];  // bits 8-9: scalars per thread of the fused recode
  k.rocprim_hist = (variant & 1024) != 0;  // bit 10: rocPRIM's own digit histogram pass (A/B)
  k.wide_stage = (variant & 2048) != 0;    // bit 11: 8-byte LDS staging in the recode scatter (A/B)
  return k;
}

// How the entries of a run are sorted: c window bits, Ws windows per scalar,
// W key windows in groups of G, `entries` in all (`mixed`: bucket-index keys).
template <class Curve>
typename MsmGpu<Curve>::SortShape MsmGpu<Curve>::sort_shape(const SortKnobs& k, unsigned c, unsigned Ws, unsigned W,
                                                            unsigned G, size_t entries, bool mixed) {
  SortShape s;
  unsigned wbits = 0;
  while ((1u << wbits) < W) ++wbits;
  s.key_bits = (G == 1) ? c : c + wbits;  // the window bits only matter within a multi-window group
  // mixed widths: the keys are bucket indices and the largest key is the
  // reserved one of the zero digits, all ones over kMixedKeyBits
  if (mixed) s.key_bits = kMixedKeyBits;
  // recode fused with the first (low byte) radix pass; one sort group only
  // (the scatter stages a block's spt x 256 x W entries in LDS, <= 128 KiB)
  s.spt = k.spt;
  s.narrow = s.key_bits <= 24 && !k.wide_stage;  // 7-byte LDS staging in the scatter
  s.scatter_lds = (size_t)s.spt * detail::kBlock * Ws * (s.narrow ? 7 : sizeof(uint64_t));
  s.fused = k.fuse_recode && G == W && s.scatter_lds <= 128 * 1024;
  s.sort_begin = s.fused ? std::min(8u, s.key_bits) : 0u;
  // onesweep passes fed with digit counts from the recode (places = the
  // 8-bit digits after the fused low byte); rocPRIM's radix_sort_keys
  // otherwise (set_variant bit 10, or other tile shapes, or > 2 places)
  s.places = (s.key_bits - s.sort_begin + 7) / 8;
  s.own_sort = s.fused && !k.rocprim_hist && s.places <= 2 && entries < (size_t(1) << 32);
  return s;
}

template <class Curve>
typename MsmGpu<Curve>::AccFields MsmGpu<Curve>::acc_fields(int variant) {
  AccFields f;
  f.tree_reduce = (variant & 4096) != 0;  // bit 12: window sums by workgroup trees (A/B)
  // BN254 G1 accumulates over the 29-bit-limb field with hand-chained products
  // (field/f29_asm.h) and product-free conversions, the next base not
  // prefetched (3 waves per SIMD): 2^26 accumulation 67.3 -> 61.0 ms, faster
  // at every size from 2^16 (profiles/r03b/ab_acc29_conv.log).  Bit 18 forces
  // the 32-bit FIPS field; bits 13 / 17 prefetch the next base in registers
  // (2 waves) / through LDS by LDS-DMA (A/B); bit 14 is the default
  const bool acc29_default = std::is_same_v<Curve, Bn254G1>;
  f.acc29 = !(variant & 262144) && ((variant & (8192 | 16384 | 131072)) != 0 || acc29_default);
  // BLS12-381 G1: the accumulation over 14 x 28-bit limbs (field/f28.h) by
  // default; bit 20 restores the 12 x 32-bit FIPS field (A/B)
  f.acc28 = std::is_same_v<Curve, Bls381G1> && !(variant & (1 << 20));
  // G2: the lane pair over the 28-bit (BLS12-381, msm/pair28.h) / 29-bit
  // (BN254, msm/pair29.h) field; bit 20 restores the FIPS pair, bit 15 the
  // one-lane FIPS kernel
  f.pair_limb = (std::is_same_v<Curve, Bls381G2> || std::is_same_v<Curve, Bn254G2>) && !(variant & (1 << 20));
  // G2: a lane pair per point with inline products by default (BLS12-381 G2
  // 2^24 accumulation 129 -> 113 ms, BN254 G2 2^22 16.3 -> 15.7 ms); bit 15
  // restores the one-lane kernel, bit 16 the pair with out-of-line 12-limb products
  f.pair_acc = !(variant & 32768);
  return f;
}

// bucket sums and pieces in the 144-byte Raw format after the 29-bit
// accumulation (not with the workgroup-tree window sums, an A/B path in R form)
// (BLS12-381 G1: 224-byte Pol28::Raw after the 28-bit accumulation, read by
// the 28-bit reductions -- not with the FIPS reductions of bit 22 or the
// two-level window sums of bit 23; every join level raw, so the level buffer
// takes the raw slot too)
// (G2 lane pairs over the limb fields: 8 raw components per point -- 448 B
// BLS12-381, 288 B BN254 -- not with the FIPS pair reductions (bit 22), the
// two-level (bit 23) or two-pass (bit 24) window sums)
template <class Curve>
typename MsmGpu<Curve>::SlotBytes MsmGpu<Curve>::slot_bytes(const AccFields& f, int variant) {
  SlotBytes s{sizeof(Point), sizeof(Point), false};
  if constexpr (std::is_same_v<Curve, Bn254G1>) {
    s.raw = f.acc29 && !f.tree_reduce;
    if (s.raw) s.slot = sizeof(acc29::Raw);
  }
  if constexpr (std::is_same_v<Curve, Bls381G1>) {
    s.raw = f.acc28 && !f.tree_reduce && !(variant & ((1 << 22) | (1 << 23)));
    if (s.raw) s.slot = s.lvl_slot = sizeof(Pol28::Raw);
  }
  if constexpr (std::is_same_v<Curve, Bn254G2> || std::is_same_v<Curve, Bls381G2>) {
    using LimbPol = std::conditional_t<std::is_same_v<Curve, Bls381G2>, PairPol28, PairPol29>;
    s.raw = f.pair_acc && f.pair_limb && !f.tree_reduce && !(variant & ((1 << 22) | (1 << 23) | (1 << 24)));
    if (s.raw) s.slot = s.lvl_slot = 8 * sizeof(typename LimbPol::F);
  }
  return s;
}

// Device bytes of the working buffers enqueue() grows for an n-point MSM
// (keys/values and their sort double buffers, sort scratch, accumulation
// pieces and chain tables, bucket and segment sums), plus 10 %.  The slot
// sizes come from slot_bytes and the plan from run_plan, as enqueue's do.
template <class Curve>
size_t MsmGpu<Curve>::work_bytes(size_t n, unsigned c, size_t batch) const {
  const MsmPlan p = run_plan(n, c);
  const size_t entries = n * p.active();
  const size_t T = (entries + p.K - 1) / p.K;
  size_t bytes = entries * 16 + entries / 2;                 // entries (x2) + onesweep scratch
  // rocPRIM's radix sort instead of the recode-fed onesweep passes (a recode
  // scatter past 128 KiB of LDS: many narrow windows; set_variant bits 7, 10):
  // its scratch holds another copy of the entries
  const unsigned W = (unsigned)(p.active() * batch), G = batch > 1 ? W : std::max(1u, std::min(p.group, W));
  if (!sort_shape(sort_knobs(variant_), p.c, p.active(), W, G, entries, p.mixed).own_sort) bytes += entries * 8;
  const SlotBytes sb = slot_bytes(acc_fields(variant_), variant_);
  const size_t slot = sb.slot;
  bytes += 2 * T * slot + (2 * T / kJoinFanLong + T + 2) * sb.lvl_slot;     // pieces + first join level
  bytes += (T + 2) * 4 * 11;                                               // flags (x2), last bucket (x2), chain tables
  bytes += (T + 2) * 4 * 12;                                               // join-level offsets (<= 12 levels of <= T chains)
  // (a batch of `batch` MSMs over n points in all keeps a block of windows per MSM)
  bytes += batch * p.total_buckets() * slot;                                // bucket sums
  // segment sums (x2), where the window sums are not one scan launch per window
  // (mixed widths: the two width classes share them, mixed_seg_sums)
  // (BN254 G1's 29-bit window sums: the one pass over both classes, pass29)
  if (sums_by_pass29(acc_fields(variant_)))
    bytes += 2 * pass29(p.mixed ? p.narrow() : W, W, p.buckets, p.seg, sb.raw).sums * sizeof(Point);
  else if (p.mixed)
    bytes += 2 * mixed_seg_sums(acc_fields(variant_), p.narrow(), p.windows, p.buckets) * sizeof(Point);
  else if (!window_sums_by_scan(acc_fields(variant_), p.buckets))
    bytes += 2 * batch * p.active() * (p.buckets / p.seg) * sizeof(Point);
  return bytes + bytes / 10;
}

template <class Curve>
size_t MsmGpu<Curve>::held_bytes() const {
  const DeviceBuffer* bufs[] = {&ents_,  &ents2_, &sort_tmp_, &scan_tmp_, &start_, &end_,
                                &cnt_,   &off_a_, &off_b_, &part_a_, &part_b_,  &seg_a_,    &seg_b_, &buckets_,
                                &hist_, &lofs_};
  size_t s = 0;
  for (const DeviceBuffer* b : bufs) s += b->capacity();
  return s;
}

// Point chunks an n-point MSM runs in so that its working set fits the
// device: the analogue of DetermineMsmDivisionsForMemory
// (icicle_msm_utils.cc:10-68; halve the chunk until the estimate is below the
// free memory) for this backend's buffers.  `resident_bytes`: what the call
// itself must keep on the device for all chunks (uploaded host inputs).
// Free memory = hipMemGetInfo + the buffers this context already holds
// (they are reused); TACHYON_MSM_MEM_LIMIT (bytes) caps it for tests.
template <class Curve>
size_t MsmGpu<Curve>::device_budget() const {
  size_t free_b = 0, total_b = 0;
  TA_HIP(hipMemGetInfo(&free_b, &total_b));
  size_t avail = free_b + held_bytes();
  if (const char* e = getenv("TACHYON_MSM_MEM_LIMIT")) avail = std::min<size_t>(avail, strtoull(e, nullptr, 10));
  return avail / 10 * 9;
}

template <class Curve>
size_t MsmGpu<Curve>::memory_divisions(size_t n, size_t resident_bytes) const {
  const size_t avail = device_budget();
  size_t d = 1;
  while (resident_bytes + work_bytes((n + d - 1) / d, force_c_) > avail) {
    if ((n + d - 1) / d <= (size_t(1) << 16))
      throw std::runtime_error("tachyon_mi355x: not enough device memory for the MSM (need " +
                               std::to_string(resident_bytes + work_bytes((n + d - 1) / d, force_c_)) + " B, have " +
                               std::to_string(avail) + " B)");
    d *= 2;
  }
  return d;
}

template <class Curve>
size_t MsmGpu<Curve>::fold_staging_bytes(size_t points, unsigned fold) {
  const size_t per_point = (size_t)fold * 5 * sizeof(F);  // XYZZ copies + prefixes
  const size_t chunk = std::max<size_t>(1, std::min(points, kFoldChunkBytes / per_point));
  return chunk * per_point;
}

template <class Curve>
unsigned MsmGpu<Curve>::fit_fold(size_t points, unsigned windows, unsigned want, size_t run_b, size_t reusable) const {
  if (points == 0 || want <= 1) return 1;
  unsigned f = 1;
  while (f * 2 <= want) f *= 2;
  // the run may reuse this context's buffers; the table and its staging are
  // new allocations, so they must also fit the free memory alone
  const size_t avail = device_budget() + reusable;
  size_t free_b = 0, total_b = 0;
  TA_HIP(hipMemGetInfo(&free_b, &total_b));
  if (const char* e = getenv("TACHYON_MSM_MEM_LIMIT")) free_b = std::min<size_t>(free_b, strtoull(e, nullptr, 10));
  const size_t avail_new = free_b / 10 * 9 + reusable;
  for (; f > 1; f /= 2) {
    if (windows % f != 0 || (uint64_t)f * points >= (uint64_t(1) << 31)) continue;
    const size_t table = fold_table_bytes(points, f), staging = fold_staging_bytes(points, f);
    if (table + staging + run_b <= avail && table + staging <= avail_new) return f;
  }
  return 1;
}

template <class Curve>
typename MsmGpu<Curve>::Point MsmGpu<Curve>::run(const void* bases, const void* scalars, size_t n) {
  last_divisions_ = 1;
  if (n == 0) {
    std::vector<Point> ws;
    run_windows(bases, scalars, n, &ws, nullptr);
    return Point::zero();
  }
  const bool host_b = !is_device_pointer(bases), host_s = !is_device_pointer(scalars);
  const size_t resident = (host_b ? n * sizeof(Aff) : 0) + (host_s ? n * sizeof(Fr) : 0);
  const size_t divisions = memory_divisions(n, resident);
  if (host_b || host_s) {
    const size_t chunks = std::max(host_chunk_count(n), divisions);
    if (chunks > 1) {
      last_divisions_ = chunks;
      return run_host_pipelined(bases, scalars, n, chunks);
    }
  }
  std::vector<Point> ws;
  MsmPlan plan;
  if (divisions == 1) {
    run_windows(bases, scalars, n, &ws, &plan);
    return combine_windows(ws, plan);
  }
  // device-resident inputs larger than the working memory: consecutive point
  // chunks, results added (the kParallelTerm sum, pippenger_adapter.h:82-113)
  last_divisions_ = divisions;
  const size_t step = (n + divisions - 1) / divisions;
  Point total = Point::zero();
  for (size_t lo = 0; lo < n; lo += step) {
    const size_t len = std::min(step, n - lo);
    run_windows(static_cast<const Aff*>(bases) + lo, static_cast<const Fr*>(scalars) + lo, len, &ws, &plan);
    total = total + combine_windows(ws, plan);
  }
  return total;
}

template <class Curve>
const typename MsmGpu<Curve>::Aff* MsmGpu<Curve>::affine_bases(const void* bases, size_t n, int form) {
  if (form < 0 || form > 3) throw std::runtime_error("tachyon_mi355x: base form must be 0 affine, 1 projective, 2 jacobian or 3 xyzz");
  if (form == 0 || n == 0) return static_cast<const Aff*>(bases);
  const size_t in_bytes = n * (form == 3 ? 4 : 3) * sizeof(F);
  const F* d_in = static_cast<const F*>(bases);
  if (!is_device_pointer(bases)) {
    d_in = static_cast<const F*>(norm_in_.ensure(in_bytes));
    TA_HIP(hipMemcpyAsync(const_cast<F*>(d_in), bases, in_bytes, hipMemcpyHostToDevice, stream_));
  }
  Aff* out = static_cast<Aff*>(norm_out_.ensure(n * sizeof(Aff)));
  F* prefix = static_cast<F*>(norm_prefix_.ensure(n * sizeof(F)));
  constexpr uint32_t kChunk = 16;
  const size_t threads = (n + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(detail::points_to_affine_kernel<F>, dim3(ceil_div(threads, detail::kBlock)), dim3(detail::kBlock),
                     0, stream_, d_in, form, out, prefix, n, kChunk);
  TA_HIP(hipGetLastError());
  TA_HIP(hipStreamSynchronize(stream_));  // the caller may hand the array to another device's stream
  return out;
}

template <class Curve>
unsigned MsmGpu<Curve>::plan_windows(size_t n) const {
  return run_plan(n, force_c_).windows;
}

template <class Curve>
unsigned MsmGpu<Curve>::fold_windows(size_t n) const {
  return MsmPlan::make(n, Fr::Config::kModulusBits, force_c_).windows;
}

// The fold table of n device-resident bases: copy k = 2^(k c W / fold) P for
// the plan of n points (forced c or the size's default), fold x n affine
// points into `out` (device).
template <class Curve>
void MsmGpu<Curve>::fold_bases(const void* bases, size_t n, unsigned fold, void* out) {
  fold_bases_c(bases, n, fold, out, MsmPlan::make(n, Fr::Config::kModulusBits, force_c_).c);
}

// ... for run_groups_folded / run_batch_folded: count x len bases (the group
// arrays back to back), the window bits of a batch of len-point MSMs
template <class Curve>
void MsmGpu<Curve>::fold_bases_groups(const void* bases, size_t len, size_t count, unsigned fold, void* out) {
  fold_bases_c(bases, len * count, fold, out, batch_window_bits(len));
}

template <class Curve>
void MsmGpu<Curve>::fold_bases_c(const void* bases, size_t n, unsigned fold, void* out, unsigned c) {
  require_gpu();
  if (!is_device_pointer(bases) || !is_device_pointer(out))
    throw std::runtime_error("tachyon_mi355x: fold_bases takes device-resident bases and output");
  const MsmPlan plan = MsmPlan::make(n, Fr::Config::kModulusBits, c);
  if (fold < 1 || plan.windows % fold != 0)
    throw std::runtime_error("tachyon_mi355x: an MSM fold must divide the plan's window count");
  // (folded base indices vi + part n share the 32-bit entry value with the sign bit)
  if ((uint64_t)fold * n >= (uint64_t(1) << 31))
    throw std::runtime_error("tachyon_mi355x: fold x points must be < 2^31 (folded base indices)");
  if (n == 0) return;
  const unsigned shift = plan.c * (plan.windows / fold);
  // chunk by chunk of points, so the XYZZ staging stays <= kFoldChunkBytes
  // whatever the table size (copy k of point i lands at out[k n + i])
  const size_t m = fold_staging_bytes(n, fold) / ((size_t)fold * 5 * sizeof(F));
  F* xyzz = static_cast<F*>(norm_in_.ensure((size_t)fold * m * 4 * sizeof(F)));
  F* prefix = static_cast<F*>(norm_prefix_.ensure((size_t)fold * m * sizeof(F)));
  constexpr uint32_t kChunk = 16;
  for (size_t lo = 0; lo < n; lo += m) {
    const size_t len = std::min(m, n - lo);
    hipLaunchKernelGGL(detail::fold_points_kernel<F>, dim3(ceil_div(len, detail::kBlock)), dim3(detail::kBlock), 0,
                       stream_, static_cast<const Aff*>(bases) + lo, len, fold, shift, xyzz);
    for (unsigned k = 0; k < fold; ++k)
      hipLaunchKernelGGL(detail::points_to_affine_kernel<F>, dim3(ceil_div(ceil_div(len, kChunk), detail::kBlock)),
                         dim3(detail::kBlock), 0, stream_, xyzz + (size_t)k * len * 4, 3,
                         static_cast<Aff*>(out) + (size_t)k * n + lo, prefix + (size_t)k * len, len, kChunk);
    TA_HIP(hipGetLastError());
  }
  TA_HIP(hipStreamSynchronize(stream_));
  // a one-time build: its XYZZ staging is not kept
  norm_in_.release();
  norm_prefix_.release();
}

// The MSM of n scalars over a fold table (fold_bases of the same n, same
// window bits): W / fold window sums instead of W.
template <class Curve>
typename MsmGpu<Curve>::Point MsmGpu<Curve>::run_folded(const void* folded_bases, const void* scalars, size_t n,
                                                        unsigned fold) {
  last_divisions_ = 1;
  if (fold <= 1) return run(folded_bases, scalars, n);
  if (!is_device_pointer(folded_bases) || !is_device_pointer(scalars))
    throw std::runtime_error("tachyon_mi355x: a folded MSM takes device-resident bases and scalars");
  if ((uint64_t)fold * n >= (uint64_t(1) << 31))
    throw std::runtime_error("tachyon_mi355x: fold x points must be < 2^31 (folded base indices)");
  if (memory_divisions(n, 0) != 1)
    throw std::runtime_error("tachyon_mi355x: a folded MSM must fit the device in one piece");
  struct Reset {
    unsigned& f;
    ~Reset() { f = 1; }
  } reset{fold_};
  fold_ = fold;
  std::vector<Point> ws;
  MsmPlan plan;
  run_windows(folded_bases, scalars, n, &ws, &plan);
  return combine_windows(ws, plan);
}

// `count` MSMs over the same `len` device-resident bases in one recode, sort,
// accumulation and reduction: MSM g's scalars are scalars[g len, (g+1) len)
// (device or host; zero scalars pad shorter ones), its windows a block of
// the key space (recode_scalar's glen), its result the Horner combination of
// its own window sums.  One launch sequence instead of `count` -- the small
// MSMs of a KZG batch commitment are latency-bound one by one.
// window size from the length of one MSM, not the batch's total (windows
// sized for the total leave count x more buckets than entries per bucket:
// 2^14 x 32 MSMs 8.4 ms at the total's c = 15), but above one MSM's own
// default: the batch's count x W windows make the per-window work count
// times larger.  c = 8 up to len 2^13, 10 from 2^14 (c swept 5..16 over len
// 2^10..2^16 x count 8..128: 8 best or within noise at len <= 2^13, 10 at
// 2^14..2^16, odd 7 and 9 behind both neighbours;
// profiles/r04c/batch_probe_c_sweep*.log)
template <class Curve>
unsigned MsmGpu<Curve>::batch_window_bits(size_t len) const {
  if (force_c_) return force_c_;
  unsigned lg = 1;
  while ((size_t(1) << lg) < len) ++lg;
  return std::max(default_window_bits(lg, Fr::Config::kModulusBits), lg <= 13 ? std::min(lg + 1, 8u) : 10u);
}

template <class Curve>
size_t MsmGpu<Curve>::max_batch_count(size_t len) const {
  if (len == 0) return 0;
  const unsigned c = batch_window_bits(len);
  const uint64_t W = (Fr::Config::kModulusBits + 1 + c - 1) / c;
  const uint64_t by_keys = (uint64_t(1) << 32) / (W << c);
  const uint64_t by_total = ((uint64_t(1) << 31) - 1) / len;
  return (size_t)std::max<uint64_t>(1, std::min<uint64_t>({4096, by_keys, by_total}));
}

template <class Curve>
std::vector<typename MsmGpu<Curve>::Point> MsmGpu<Curve>::run_batch(const void* bases, const void* scalars,
                                                                    size_t len, size_t count) {
  return run_batch_impl(bases, scalars, len, count, false);
}

// `count` MSMs of `len` points each with their OWN bases -- MSM g over
// bases[g len, (g+1) len) and scalars[g len, (g+1) len) -- in one launch
// sequence, as run_batch (the recode's base index keeps the global i).  The
// Groth16 prover's A and witness + h MSMs run this way.
template <class Curve>
std::vector<typename MsmGpu<Curve>::Point> MsmGpu<Curve>::run_groups(const void* bases, const void* scalars,
                                                                     size_t len, size_t count) {
  return run_batch_impl(bases, scalars, len, count, true);
}

// run_groups over a fold table of the count x len bases (fold_bases_groups)
template <class Curve>
std::vector<typename MsmGpu<Curve>::Point> MsmGpu<Curve>::run_groups_folded(const void* folded_bases,
                                                                            const void* scalars, size_t len,
                                                                            size_t count, unsigned fold) {
  if (!is_device_pointer(folded_bases))
    throw std::runtime_error("tachyon_mi355x: a folded MSM takes a device-resident fold table");
  return run_batch_impl(folded_bases, scalars, len, count, true, fold);
}

template <class Curve>
std::vector<typename MsmGpu<Curve>::Point> MsmGpu<Curve>::run_batch_impl(const void* bases, const void* scalars,
                                                                         size_t len, size_t count, bool distinct,
                                                                         unsigned fold) {
  std::vector<Point> res(count, Point::zero());
  if (count == 0 || len == 0) return res;
  if (count == 1 && fold <= 1) {
    res[0] = run(bases, scalars, len);
    return res;
  }
  if (fold > 1 && !is_device_pointer(scalars))
    throw std::runtime_error("tachyon_mi355x: a folded MSM batch takes device-resident scalars");
  if (!is_device_pointer(bases)) throw std::runtime_error("tachyon_mi355x: run_batch needs device-resident bases");
  const size_t total = len * count;
  if (total >= (size_t(1) << 31) || count > 4096)
    throw std::runtime_error("tachyon_mi355x: MSM batch too large (< 2^31 scalars, <= 4096 MSMs)");
  if (fold > 1 && (uint64_t)fold * total >= (uint64_t(1) << 31))
    throw std::runtime_error("tachyon_mi355x: fold x points must be < 2^31 (folded base indices)");
  // (window size: batch_window_bits)
  struct Reset {
    MsmGpu* m;
    unsigned c;
    ~Reset() {
      m->batch_ = 1;
      m->batch_distinct_ = false;
      m->force_c_ = c;
      m->fold_ = 1;
    }
  } reset{this, force_c_};
  force_c_ = batch_window_bits(len);
  batch_distinct_ = distinct;
  batch_ = (unsigned)count;
  fold_ = std::max(1u, fold);
  last_divisions_ = 1;
  std::vector<Point> ws;
  MsmPlan plan;
  run_windows(bases, scalars, total, &ws, &plan);
  // each MSM's Horner combination of its windows on the host (W c doublings
  // apiece), spread over a few host threads for larger batches
  const unsigned Ws = fold_ > 1 ? plan.windows / fold_ : plan.active();  // window sums per MSM
  auto combine = [&](size_t g0, size_t g1) {
    for (size_t g = g0; g < g1; ++g) {
      std::vector<Point> one(ws.begin() + g * Ws, ws.begin() + (g + 1) * Ws);
      res[g] = combine_windows(one, plan);
    }
  };
  const size_t nth = std::min<size_t>({count / 4, 16, std::max(1u, std::thread::hardware_concurrency())});
  if (nth <= 1) {
    combine(0, count);
  } else {
    std::vector<std::thread> th;
    const size_t step = (count + nth - 1) / nth;
    for (size_t g0 = 0; g0 < count; g0 += step) th.emplace_back(combine, g0, std::min(count, g0 + step));
    for (auto& t : th) t.join();
  }
  return res;
}

// The windows [w_begin, w_end) alone (PippengerBase::AccumulateWindowSums
// restricted to them): Horner over the range, then c * w_begin doublings.
template <class Curve>
typename MsmGpu<Curve>::Point MsmGpu<Curve>::run_window_range(const void* bases, const void* scalars, size_t n,
                                                              unsigned w_begin, unsigned w_end) {
  struct Reset {
    MsmGpu* m;
    ~Reset() { m->range_begin_ = 0; m->range_end_ = ~0u; }
  } reset{this};
  range_begin_ = w_begin;
  range_end_ = w_end;
  last_divisions_ = 1;
  std::vector<Point> ws;
  MsmPlan plan;
  // the window range of every point chunk run() would use for memory
  // (DetermineMsmDivisionsForMemory), partials added; host inputs stay on the
  // host and each chunk uploads its own slice (counted as resident: a
  // conservative bound).  The window bits must not depend on the chunk size,
  // so the whole input's plan is forced on the chunks.
  if (n == 0) {
    run_windows(bases, scalars, 0, &ws, &plan);
    return Point::zero();
  }
  const size_t resident = (is_device_pointer(bases) ? 0 : n * sizeof(Aff)) +
                          (is_device_pointer(scalars) ? 0 : n * sizeof(Fr));
  const size_t divisions = memory_divisions(n, resident);
  struct RestoreC {
    MsmGpu* m;
    unsigned c;
    ~RestoreC() { m->force_c_ = c; }
  } restore_c{this, force_c_};
  if (divisions > 1 && !force_c_) force_c_ = MsmPlan::make(n, Fr::Config::kModulusBits).c;
  last_divisions_ = divisions;
  const size_t step = (n + divisions - 1) / divisions;
  Point total = Point::zero();
  for (size_t lo = 0; lo < n; lo += step) {
    const size_t len = std::min(step, n - lo);
    run_windows(static_cast<const Aff*>(bases) + lo, static_cast<const Fr*>(scalars) + lo, len, &ws, &plan);
    if (plan.active() == 0) return Point::zero();
    Point p = combine_windows(ws, plan);
    for (unsigned k = 0; k < plan.c * plan.w_begin; ++k) p = p.dbl();
    total = total + p;
  }
  return total;
}

}  // namespace tachyon_amd::msm
