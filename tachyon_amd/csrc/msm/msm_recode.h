// MSM stage 1, recode: scalars -> signed digits -> 64-bit (key, val) entries, plain or
// fused with the first radix pass (part of msm_impl.h, which includes the stages in order).
#pragma once

namespace tachyon_amd::msm {
namespace detail {
namespace {  // internal linkage: every per-curve TU gets its own copy

// ---------------------------------------------------------------------------
// recode: Montgomery scalar -> canonical -> signed base-2^c digits
// (FillDigits, pippenger.h:28-51: digits in [-2^(c-1), 2^(c-1)), carry into
// the top digit; W*c >= bits+1 keeps the top digit in [0, 2^(c-1)]).
// key = window << c | |digit| (digit 0 = no contribution), so one radix sort
// over all windows orders the entries by (window, bucket) and every window
// keeps its slice [w*n, (w+1)*n); val = point index | sign << 31.
// An entry is one 64-bit word, key << 32 | val: the radix passes sort words
// on bits [32, 32 + key bits) (keys-only, one array) and the accumulation
// reads one 8-byte word per entry.
// Signed c-bit digits of one scalar, window by window: emit(w, key, val).
// Windows [w0, w0 + wr) of W are emitted, as local windows 0 .. wr-1 (the
// lower windows still run for their carries).
template <class Fr, class Emit>
// glen > 0 (a batch of MSMs, run_batch / run_groups): scalar i belongs to
// MSM g = i / glen, its windows are g * wr .. g * wr + wr - 1 of the key space
// and its base index is i - g * gstep (gstep = glen: the MSMs share one base
// array; gstep = 0: MSM g has its own bases at [g glen, (g+1) glen)).
// fold_w > 0 (run_folded: F = W / fold_w copies of the bases, copy k =
// 2^(k c fold_w) P): window w goes to key window w mod fold_w (of MSM g's
// block g fold_w in a batch) and to copy w / fold_w, base index
// vi + (w / fold_w) fold_n (fold_n = the length of one copy).
// narrow < W (mixed widths, MsmPlan::make_mixed: a plain run, all windows, no
// batch, no fold): windows [narrow, W) are c + 1 bits wide and the key is the
// bucket's index over all windows, koff(w) + |digit| - 1, with koff(w) = (w +
// max(0, w - narrow)) 2^(c-1) buckets below window w; a zero digit gets the
// reserved key kMixedNoKey (it sorts last).  bucket_of_key decodes both forms.
__device__ __forceinline__ void recode_scalar(const Fr& scalar, uint32_t i, unsigned c, unsigned W, unsigned w0,
                                              unsigned wr, Emit emit, uint32_t glen = 0, uint32_t gstep = 0,
                                              uint32_t fold_w = 0, uint32_t fold_n = 0, uint32_t narrow = ~0u) {
  constexpr int N = Fr::N;
  Fr s = scalar.from_mont();
  uint32_t limbs[N];
#pragma unroll
  for (int k = 0; k < N; ++k) limbs[k] = s.v[k];
  const unsigned c_lo = c;
  uint32_t mask = (1u << c) - 1;
  uint32_t half = 1u << (c - 1);
  uint32_t gw = 0, vi = i;
  if (glen) {
    const uint32_t g = i / glen;
    gw = g * (fold_w ? fold_w : wr);
    vi = i - g * gstep;
  }
  uint32_t carry = 0;
  for (unsigned w = 0; w < w0 + wr; ++w) {
    if (w == narrow) {  // the wide windows from here on
      c = c_lo + 1;
      mask = (1u << c) - 1;
      half = 1u << (c - 1);
    }
    uint32_t coeff = (limbs[0] & mask) + carry;
    // shift the scalar right by c (c < 32), constant-indexed limbs only: one
    // funnel shift (v_alignbit_b32) per limb
#pragma unroll
    for (int k = 0; k < N - 1; ++k) limbs[k] = __builtin_amdgcn_alignbit(limbs[k + 1], limbs[k], c);
    limbs[N - 1] >>= c;
    uint32_t key, sign;
    if (w + 1 < W) {
      carry = (coeff + half) >> c;
      int32_t d = (int32_t)coeff - (int32_t)(carry << c);
      sign = d < 0 ? kSignBit : 0u;
      key = (uint32_t)(d < 0 ? -d : d);
    } else {
      key = coeff;  // top digit, carry folded in, non-negative
      sign = 0;
    }
    if (narrow != ~0u) {
      const uint32_t koff = (w + (w > narrow ? w - narrow : 0u)) << (c_lo - 1);
      emit(w, key ? koff + key - 1 : kMixedNoKey, vi | sign);
    } else if (fold_w) {
      const uint32_t part = w / fold_w;
      emit(w, ((gw + w - part * fold_w) << c) | key, (vi + part * fold_n) | sign);
    } else if (w >= w0) {
      emit(w - w0, ((gw + w - w0) << c) | key, vi | sign);
    }
  }
}

__device__ __forceinline__ uint64_t make_entry(uint32_t key, uint32_t val) { return (uint64_t)key << 32 | val; }
__device__ __forceinline__ uint32_t entry_key(uint64_t e) { return (uint32_t)(e >> 32); }
__device__ __forceinline__ uint32_t entry_val(uint64_t e) { return (uint32_t)e; }

// The bucket of a key, or kNoBucket for a zero digit.  c > 0: the combined key
// window << c | |digit| of uniform c-bit windows, bucket w 2^(c-1) + |digit| -
// 1.  c == 0 (mixed widths): the key is the bucket, the reserved key is none.
// c is a kernel argument, so the choice is wave-uniform.
__device__ __forceinline__ uint32_t bucket_of_key(uint32_t key, uint32_t c) {
  if (c == 0) return key == kMixedNoKey ? kNoBucket : key;
  const uint32_t d = key & ((1u << c) - 1);
  return d ? ((key >> c) << (c - 1)) + (d - 1) : kNoBucket;
}

template <class Fr>
__global__ __launch_bounds__(kBlock) void recode_kernel(const Fr* __restrict__ scalars, uint32_t n,
                                                        unsigned c, unsigned W, unsigned w0, unsigned wr,
                                                        uint64_t* __restrict__ ents, uint32_t glen, uint32_t gstep,
                                                        uint32_t fold_w, uint32_t fold_n, uint32_t narrow) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  recode_scalar(
      scalars[i], i, c, W, w0, wr,
      [&](unsigned w, uint32_t key, uint32_t val) { ents[(size_t)w * n + i] = make_entry(key, val); }, glen, gstep,
      fold_w, fold_n, narrow);
}

// Recode fused with the first radix pass (key bits 0..7), in two launches:
// recode_hist_kernel counts, per block of spt x 256 scalars, the entries
// of each low-byte bin (LDS atomics) into the block's row hist[block * 256 +
// bin]; bin_chunk_sums / bin_chunk_scan / bin_offsets_kernel turn the rows
// into every (block, bin)'s global slot (bin-major order: all of bin 0's
// entries first, blocks in order within a bin), written as rows again, and
// recode_scatter_kernel recomputes the digits and
// writes every (key, val) to its bin's slot (the rank inside the block's run
// from LDS atomics).  This pass need not be stable -- the later stable passes
// over bits 8.. keep the bin grouping, and the order inside a bucket does not
// change the bucket's sum -- so it replaces the recode's 8-byte write plus one
// full onesweep pass (read + write + histogram read) with two reads of the
// 32-byte scalars and one write.
constexpr unsigned kRecodeSpt = 2;  // default scalars per thread of the fused recode

// LDS bin ranks with one atomic per wave when every active lane hits the
// same bin -- NonUniform(n, 1) scalars (variable_base_msm_test_set.h:43-53),
// small scalars' empty high windows -- instead of 64 serialised atomics on
// one address (2^26 NonUniform recode 12.8 -> see DESIGN.md); otherwise one
// atomic per lane.  The test is wave-uniform (ballots), so no divergence.
// (recode_hist_kernel makes the same test once per entry for its three bins.)
// A returning add of 1: this lane's slot in bin's run
__device__ __forceinline__ uint32_t lds_rank(uint32_t* cur, uint32_t bin) {
  const uint32_t b0 = __builtin_amdgcn_readfirstlane(bin);
  const uint64_t active = __ballot(1);
  if (__ballot(bin == b0) == active) {
    const uint32_t leader = (uint32_t)(__ffsll((unsigned long long)active) - 1);
    const uint32_t below = (uint32_t)__popcll(active & ((1ull << __lane_id()) - 1));
    uint32_t base = 0;
    if (__lane_id() == leader) base = atomicAdd(&cur[b0], (uint32_t)__popcll(active));
    return __shfl(base, leader, 64) + below;
  }
  return atomicAdd(&cur[bin], 1u);
}

// Places > 0 (key bits 8..15, 16..23): with `places` > 0 the kernel also
// counts those digits per block, into later[((p - 1) * nblocks + block) * 256
// + bin], so the onesweep passes over those places need no histogram pass of
// their own over the W*n entries (digit_count_kernel + digit_scan_kernel turn
// the counts into rocPRIM's global digit offsets).
template <class Fr>
__global__ __launch_bounds__(kBlock) void recode_hist_kernel(const Fr* __restrict__ scalars, uint32_t n, unsigned c,
                                                             unsigned W, unsigned w0, unsigned wr,
                                                             uint32_t nblocks, uint32_t spt, uint32_t places,
                                                             uint32_t* __restrict__ hist,
                                                             uint32_t* __restrict__ later,
                                                             uint4* __restrict__ zero, size_t zero_n, uint32_t glen,
                                                             uint32_t gstep, uint32_t fold_w, uint32_t fold_n,
                                                             uint32_t narrow) {
  // cnt2: the third place's counts (key bits 16..23) in four copies, one per
  // lane & 3, 264 words apart: those bits are the window (the same in every
  // lane of a step) and the digit's top bits, a handful of values per wave --
  // one copy gave up to 8 lanes per address in a 32-lane atomic group (8-way
  // conflicts); with the copies on distinct banks a group spreads over 4x the
  // addresses.  A wave-uniform value takes one atomic (c <= 16: the bits are
  // the window alone).
  constexpr uint32_t kCopy = 264;
  __shared__ uint32_t cnt[2][256];
  __shared__ uint32_t cnt2[4 * kCopy];
  const uint32_t t = threadIdx.x;
  // the bucket sums start as the identity (all-zero words): cleared here, not by a memset launch
  for (size_t i = (size_t)blockIdx.x * kBlock + t; i < zero_n; i += (size_t)nblocks * kBlock) zero[i] = uint4{0, 0, 0, 0};
  cnt[0][t] = 0;
  cnt[1][t] = 0;
  for (uint32_t j = t; j < 4 * kCopy; j += kBlock) cnt2[j] = 0;
  __syncthreads();
  for (uint32_t k = 0; k < spt; ++k) {
    const uint32_t i = blockIdx.x * spt * kBlock + k * kBlock + t;
    if (i < n)
      recode_scalar(scalars[i], i, c, W, w0, wr, [&](unsigned, uint32_t key, uint32_t) {
        // one wave-uniformity test for the entry's three bins (equal keys
        // have equal bins): NonUniform inputs take one atomic per wave
        const uint32_t k0 = __builtin_amdgcn_readfirstlane(key);
        const uint64_t active = __ballot(1);
        const uint32_t leader = (uint32_t)(__ffsll((unsigned long long)active) - 1);
        if (__ballot(key == k0) == active) {
          if (__lane_id() == leader) {
            const uint32_t m = (uint32_t)__popcll(active);
            atomicAdd(&cnt[0][k0 & 255], m);
            if (places > 0) atomicAdd(&cnt[1][(k0 >> 8) & 255], m);
            if (places > 1) atomicAdd(&cnt2[(k0 >> 16) & 255], m);
          }
        } else {
          atomicAdd(&cnt[0][key & 255], 1u);
          if (places > 0) atomicAdd(&cnt[1][(key >> 8) & 255], 1u);
          if (places > 1) {
            const uint32_t b2 = (key >> 16) & 255, v0 = __builtin_amdgcn_readfirstlane(b2);
            if (__ballot(b2 == v0) == active) {
              if (__lane_id() == leader) atomicAdd(&cnt2[v0], (uint32_t)__popcll(active));
            } else {
              atomicAdd(&cnt2[(__lane_id() & 3) * kCopy + b2], 1u);
            }
          }
        }
      }, glen, gstep, fold_w, fold_n, narrow);
  }
  __syncthreads();
  hist[(size_t)blockIdx.x * 256 + t] = cnt[0][t];  // one coalesced 1 KiB row per block
  if (places > 0) later[(size_t)blockIdx.x * 256 + t] = cnt[1][t];
  if (places > 1)
    later[((size_t)nblocks + blockIdx.x) * 256 + t] = cnt2[t] + cnt2[kCopy + t] + cnt2[2 * kCopy + t] + cnt2[3 * kCopy + t];
}

// counts[q * 256 + bin] += the later-place counts of a chunk of recode blocks
// (grid: chunks x places; one coalesced 1 KiB row per block)
__global__ __launch_bounds__(kBlock) void digit_count_kernel(const uint32_t* __restrict__ later, uint32_t nblocks,
                                                             uint32_t per_chunk, uint32_t* __restrict__ counts) {
  const uint32_t q = blockIdx.y, t = threadIdx.x;
  const uint32_t b0 = blockIdx.x * per_chunk, b1 = min(nblocks, b0 + per_chunk);
  const uint32_t* rows = later + (size_t)q * nblocks * 256;
  uint32_t acc = 0;
  for (uint32_t b = b0; b < b1; ++b) acc += rows[(size_t)b * 256 + t];
  if (acc) atomicAdd(&counts[q * 256 + t], acc);
}

// exclusive prefix sums of each place's 256 digit counts (one workgroup per
// place): rocPRIM's global digit offsets, place q at [q * 256, (q + 1) * 256)
__global__ __launch_bounds__(kBlock) void digit_scan_kernel(const uint32_t* __restrict__ counts,
                                                            uint32_t* __restrict__ offsets) {
  const uint32_t q = blockIdx.x, t = threadIdx.x;
  const uint32_t mine = counts[q * 256 + t];
  uint32_t v = mine;  // 4 waves x 64 lanes
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if ((t & 63) >= (uint32_t)d) v += u;
  }
  __shared__ uint32_t wave_tot[kBlock / 64];
  if ((t & 63) == 63) wave_tot[t >> 6] = v;
  __syncthreads();
  uint32_t add = 0;
  for (uint32_t w = 0; w < (t >> 6); ++w) add += wave_tot[w];
  offsets[q * 256 + t] = v - mine + add;
}

// The fused recode's slots from its per-block bin rows (hist[block][bin],
// 256 bins): slot(block, bin) = sum_{bin' < bin} total(bin') + sum_{block' <
// block} hist[block'][bin] -- the exclusive scan of the bin-major flattening,
// computed over coalesced 1 KiB rows (the bin-major array itself would be
// written and read one 4-byte word per 64-byte line by the recode kernels).
// Chunks of per_chunk consecutive blocks: csum[chunk][bin] = the chunk's sum.
__global__ __launch_bounds__(kBlock) void bin_chunk_sums_kernel(const uint32_t* __restrict__ rows, uint32_t nblocks,
                                                                uint32_t per_chunk, uint32_t* __restrict__ csum) {
  const uint32_t t = threadIdx.x, b0 = blockIdx.x * per_chunk, b1 = min(nblocks, b0 + per_chunk);
  uint32_t acc = 0;
  for (uint32_t b = b0; b < b1; ++b) acc += rows[(size_t)b * 256 + t];
  csum[(size_t)blockIdx.x * 256 + t] = acc;
}

// workgroup = one bin: cpre[chunk][bin] = exclusive prefix of csum[.][bin]
// over the chunks, total[bin] = the bin's count (a block scan per 256 chunks)
__global__ __launch_bounds__(kBlock) void bin_chunk_scan_kernel(const uint32_t* __restrict__ csum, uint32_t chunks,
                                                                uint32_t* __restrict__ cpre,
                                                                uint32_t* __restrict__ total) {
  const uint32_t bin = blockIdx.x, t = threadIdx.x;
  __shared__ uint32_t wave_tot[kBlock / 64];
  uint32_t carry = 0;
  for (uint32_t c0 = 0; c0 < chunks; c0 += kBlock) {
    const uint32_t ch = c0 + t;
    const uint32_t mine = ch < chunks ? csum[(size_t)ch * 256 + bin] : 0u;
    uint32_t v = mine;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(v, d, 64);
      if ((t & 63) >= (uint32_t)d) v += u;
    }
    if ((t & 63) == 63) wave_tot[t >> 6] = v;
    __syncthreads();
    uint32_t add = carry, tile = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
      if (w < (t >> 6)) add += wave_tot[w];
      tile += wave_tot[w];
    }
    if (ch < chunks) cpre[(size_t)ch * 256 + bin] = v - mine + add;
    carry += tile;
    __syncthreads();  // wave_tot is rewritten by the next tile
  }
  if (t == 0) total[bin] = carry;
}

// workgroup = one chunk, thread = one bin: the chunk's rows of slots
__global__ __launch_bounds__(kBlock) void bin_offsets_kernel(const uint32_t* __restrict__ rows, uint32_t nblocks,
                                                             uint32_t per_chunk, const uint32_t* __restrict__ cpre,
                                                             const uint32_t* __restrict__ total,
                                                             uint32_t* __restrict__ off) {
  const uint32_t t = threadIdx.x, b0 = blockIdx.x * per_chunk, b1 = min(nblocks, b0 + per_chunk);
  // exclusive scan of the 256 bin totals: this bin's base
  const uint32_t mine = total[t];
  uint32_t v = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if ((t & 63) >= (uint32_t)d) v += u;
  }
  __shared__ uint32_t wave_tot[kBlock / 64];
  if ((t & 63) == 63) wave_tot[t >> 6] = v;
  __syncthreads();
  uint32_t run = v - mine + cpre[(size_t)blockIdx.x * 256 + t];
  for (uint32_t w = 0; w < (t >> 6); ++w) run += wave_tot[w];
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t c = rows[(size_t)b * 256 + t];
    off[(size_t)b * 256 + t] = run;
    run += c;
  }
}

// kNarrow: keys of <= 24 bits are staged as 7 bytes (val, key >> 8, bin),
// 47 KiB instead of 53 KiB per block at 13 windows -- three workgroups per
// CU instead of two.
template <class Fr, bool kNarrow>
__global__ __launch_bounds__(kBlock) void recode_scatter_kernel(const Fr* __restrict__ scalars, uint32_t n,
                                                                unsigned c, unsigned W, unsigned w0, unsigned wr,
                                                                uint32_t nblocks, uint32_t spt,
                                                                const uint32_t* __restrict__ hist,
                                                                const uint32_t* __restrict__ off,
                                                                uint64_t* __restrict__ ents, uint32_t glen,
                                                                uint32_t gstep, uint32_t fold_w, uint32_t fold_n,
                                                                uint32_t narrow) {
  // the block's entries are binned in LDS first, then written out bin run by
  // bin run, so consecutive lanes store to consecutive addresses
  extern __shared__ uint64_t lds_u64[];
  uint64_t* lents = lds_u64;                      // spt * kBlock * wr (wide)
  uint32_t* lvals = reinterpret_cast<uint32_t*>(lds_u64);  // narrow: vals, then the 16-bit key tops
  uint16_t* lkeys = reinterpret_cast<uint16_t*>(lvals + (size_t)spt * kBlock * wr);
  uint8_t* lbins = reinterpret_cast<uint8_t*>(lkeys + (size_t)spt * kBlock * wr);
  __shared__ uint32_t base[256], loff[256], cur[256];
  const uint32_t t = threadIdx.x;
  base[t] = off[(size_t)blockIdx.x * 256 + t];
  const uint32_t mine = hist[(size_t)blockIdx.x * 256 + t];
  // exclusive scan of the block's 256 bin counts (4 waves x 64 lanes)
  uint32_t v = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if ((t & 63) >= (uint32_t)d) v += u;
  }
  __shared__ uint32_t wave_tot[kBlock / 64];
  if ((t & 63) == 63) wave_tot[t >> 6] = v;
  __syncthreads();
  uint32_t add = 0;
  for (uint32_t w = 0; w < (t >> 6); ++w) add += wave_tot[w];
  loff[t] = v - mine + add;
  cur[t] = 0;
  __syncthreads();
  for (uint32_t k = 0; k < spt; ++k) {
    const uint32_t i = blockIdx.x * spt * kBlock + k * kBlock + t;
    if (i < n)
      recode_scalar(scalars[i], i, c, W, w0, wr, [&](unsigned, uint32_t key, uint32_t val) {
        const uint32_t bin = key & 255;
        const uint32_t p = loff[bin] + lds_rank(cur, bin);
        if constexpr (kNarrow) {
          lvals[p] = val;
          lkeys[p] = (uint16_t)(key >> 8);
          lbins[p] = (uint8_t)bin;
        } else {
          lents[p] = make_entry(key, val);
        }
      }, glen, gstep, fold_w, fold_n, narrow);
  }
  __syncthreads();
  const uint32_t total = loff[255] + cur[255];
  if constexpr (kNarrow) {
    for (uint32_t p = t; p < total; p += kBlock) {
      const uint32_t bin = lbins[p];
      ents[base[bin] + (p - loff[bin])] = make_entry(((uint32_t)lkeys[p] << 8) | bin, lvals[p]);
    }
  } else {
    for (uint32_t p = t; p < total; p += kBlock) {
      const uint64_t e = lents[p];
      const uint32_t bin = entry_key(e) & 255;
      ents[base[bin] + (p - loff[bin])] = e;
    }
  }
}

}  // namespace
}  // namespace detail
}  // namespace tachyon_amd::msm
