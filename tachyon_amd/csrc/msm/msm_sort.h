// MSM stage 2, sort: the rocPRIM onesweep configurations and the recode-fed onesweep pass
// (part of msm_impl.h).
#pragma once

namespace tachyon_amd::msm {

// rocPRIM keys-only onesweep sort of the 64-bit entries on the key bits
// [begin_bit, end_bit) (entry bits 32 + those).  8-bit digits; the tile
// shape is set_variant bits 4-5 (A/B): 0 = 1024 threads x 8 items, 1 =
// rocPRIM's gfx950 default for 64-bit keys, 2 = 512 x 16, 3 = 1024 x 12.
// 2^26 sort: 11.0 / 12.2 / 11.7 ms (2^24: 2.72 / 3.07 / 2.95).  Sorting
// (key, val) u32 pairs took 12.7 ms and the accumulation read two words per
// entry: 2^26 MSM 95.0 -> 92.0 ms with the 64-bit entries.
template <unsigned Threads, unsigned Items>
using OnesweepCfg = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<Threads, Items>, rocprim::kernel_config<Threads, Items>,
                                        8, rocprim::block_radix_rank_algorithm::match>>;

// One rocPRIM onesweep pass (keys only, 1024 x 8 tiles, 8-bit digits) over
// entry bits [bit, end_bit) from `in` to `out`, with the global digit offsets
// given: radix_sort_keys would first read all W*n entries once more for its
// digit histograms (2.4 ms at 2^26); the fused recode counts those digits as
// it computes them (recode_hist_kernel).  rocPRIM's own iteration entry point
// (lookback reset, ordered block ids, batching) does the rest.
namespace {
template <unsigned Threads, unsigned Items, rocprim::block_radix_rank_algorithm Rank>
using MsmOnesweep = rocprim::radix_sort_onesweep_config<rocprim::kernel_config<Threads, Items>,
                                                        rocprim::kernel_config<Threads, Items>, 8, Rank>;
using MsmBlockId = rocprim::detail::block_id_wrapper<unsigned int, true>;
constexpr uint32_t kOnesweepMinTile = 256 * 16;  // smallest tile below (sizes the lookback states)

template <class Cfg>
hipError_t onesweep_pass_cfg(const uint64_t* in, uint64_t* out, uint32_t size, unsigned bit, unsigned end_bit,
                             uint32_t* digit_offsets, uint32_t* offsets_tmp, void* lookback, void* block_id,
                             hipStream_t s) {
  rocprim::empty_type* none = nullptr;
  return rocprim::detail::radix_sort_onesweep_iteration<Cfg, false>(
      in, static_cast<uint64_t*>(nullptr), out, none, none, none, size, digit_offsets, offsets_tmp,
      static_cast<rocprim::detail::onesweep_lookback_state*>(lookback), true, true, rocprim::identity_decomposer{},
      bit, end_bit, MsmBlockId::create(block_id), s, false);
}

// tile shapes (set_variant bits 4-5, A/B): 0 = 1024 x 8 warp-match ranking
hipError_t onesweep_pass(unsigned cfg, const uint64_t* in, uint64_t* out, uint32_t size, unsigned bit,
                         unsigned end_bit, uint32_t* digit_offsets, uint32_t* offsets_tmp, void* lookback,
                         void* block_id, hipStream_t s) {
  using R = rocprim::block_radix_rank_algorithm;
  switch (cfg) {
    case 1:
      return onesweep_pass_cfg<MsmOnesweep<512, 8, R::match>>(in, out, size, bit, end_bit, digit_offsets,
                                                                offsets_tmp, lookback, block_id, s);
    case 2:
      return onesweep_pass_cfg<MsmOnesweep<256, 16, R::match>>(in, out, size, bit, end_bit, digit_offsets,
                                                                 offsets_tmp, lookback, block_id, s);
    case 3:
      return onesweep_pass_cfg<MsmOnesweep<1024, 12, R::match>>(in, out, size, bit, end_bit, digit_offsets,
                                                                  offsets_tmp, lookback, block_id, s);
#ifdef TACHYON_TUNING_KNOBS  // more tile shapes for A/B (TACHYON_ONESWEEP_CFG=4, 5; tuning builds only)
    case 4:
      return onesweep_pass_cfg<MsmOnesweep<1024, 16, R::match>>(in, out, size, bit, end_bit, digit_offsets,
                                                                  offsets_tmp, lookback, block_id, s);
    case 5:
      return onesweep_pass_cfg<MsmOnesweep<512, 16, R::match>>(in, out, size, bit, end_bit, digit_offsets,
                                                                 offsets_tmp, lookback, block_id, s);
#endif
    default:
      return onesweep_pass_cfg<MsmOnesweep<1024, 8, R::match>>(in, out, size, bit, end_bit, digit_offsets,
                                                                 offsets_tmp, lookback, block_id, s);
  }
}
}  // namespace

}  // namespace tachyon_amd::msm
