// Challenger::Grind (challenger.h:87-122) on the GPU: the smallest witness w in
// [from, to) whose observation makes the next sample's low `bits` bits zero.
// The transcript stays on the host (challenger_bb.h); the search is the kernel
// of grind_bb.hip.
#pragma once
#include <cstdint>

#include "../common/hip_util.h"
#include "challenger_bb.h"

namespace tachyon_amd::fri {

inline constexpr uint64_t kGrindMinChunk = uint64_t(1) << 16;   // candidates of the smallest launch
inline constexpr uint64_t kGrindMaxChunk = uint64_t(1) << 24;   // about 3 ms of permutations

inline bool grind_args_ok(unsigned bits, uint64_t from, uint64_t to) {
  return bits <= kMaxSampleBits && from < to && to <= bb31::kP;
}

// Candidates of the first launch: four times the expected work 2^bits, which
// holds a witness with probability 1 - e^-4, within the two bounds above.
inline uint64_t grind_first_chunk(unsigned bits) {
  const uint64_t want = uint64_t(4) << bits;
  return want < kGrindMinChunk ? kGrindMinChunk : want > kGrindMaxChunk ? kGrindMaxChunk : want;
}

// False, with the challenger unchanged, when the arguments are refused or the
// range holds no witness.  On success *witness_out is the Montgomery word and
// the challenger stands where check_witness(bits, witness) leaves it.
// `scratch` provides the device word of the minimum; *launches, if given,
// receives the number of kernel launches.  One copy-back and one wait per
// launch.
bool grind(DuplexChallenger& challenger, unsigned bits, uint64_t from, uint64_t to, uint32_t* witness_out,
           DeviceBuffer& scratch, hipStream_t stream, unsigned* launches = nullptr);

}  // namespace tachyon_amd::fri
