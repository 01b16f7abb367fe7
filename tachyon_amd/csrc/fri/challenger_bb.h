// DuplexChallenger<Poseidon2, 16, R> over BabyBear (duplex_challenger.h:33-65,
// challenger.h:87-122) on the host: plain C++ with no HIP dependency.  Words are
// canonical Montgomery words (field/bb31.h).
//
// The state is 16 words, the input buffer holds fewer than `rate` words between
// calls (a buffer that fills is duplexed at once) and the output buffer is what
// is left of the state the last duplex produced; samples pop from its back.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../field/bb31.h"
#include "../hash/poseidon2_bb.h"

namespace tachyon_amd::fri {

inline constexpr unsigned kChallengerWidth = 16;
inline constexpr unsigned kMaxSampleBits = 30;  // the reference requires 2^bits < p
// words written by DuplexChallenger::dump(): state, then the length and the 16
// slots of the input buffer, then those of the output buffer
inline constexpr size_t kChallengerStateWords = 16 + 2 * (1 + 16);

inline bool challenger_rate_ok(unsigned rate) { return rate >= 1 && rate <= kChallengerWidth; }

class DuplexChallenger {
 public:
  DuplexChallenger(int external, unsigned rate) : external_(external), rate_(rate) {}

  int external() const { return external_; }
  unsigned rate() const { return rate_; }
  const uint32_t* state() const { return state_; }
  unsigned num_inputs() const { return num_in_; }
  const uint32_t* inputs() const { return in_; }
  unsigned num_outputs() const { return num_out_; }

  // false, and nothing is observed, when a word is not below p
  bool observe(const uint32_t* values, size_t count) {
    for (size_t i = 0; i < count; ++i)
      if (values[i] >= bb31::kP) return false;
    for (size_t i = 0; i < count; ++i) observe_one(values[i]);
    return true;
  }

  uint32_t sample() {
    if (num_in_ != 0 || num_out_ == 0) duplex();
    return out_[--num_out_];
  }

  // SampleExtElement: c0 first
  void sample_ext(uint32_t* out4) {
    for (int k = 0; k < 4; ++k) out4[k] = sample();
  }

  // the low `bits` bits of the sample's canonical value; bits <= kMaxSampleBits
  uint32_t sample_bits(unsigned bits) { return bb31::from_mont(sample()) & ((uint32_t(1) << bits) - 1); }

  // CheckWitness: the transcript advances whether or not the witness is good
  bool check_witness(unsigned bits, uint32_t witness) {
    observe_one(witness);
    return sample_bits(bits) == 0;
  }

  // Grind's view of the transcript: observing a candidate and sampling after it
  // costs one permutation, of the state with the input buffer and the candidate
  // at `slot` laid over it, whether or not the candidate fills the rate; the
  // sample is word 15 of the result.
  unsigned grind_base(uint32_t* base16) const {
    for (unsigned i = 0; i < kChallengerWidth; ++i) base16[i] = i < num_in_ ? in_[i] : state_[i];
    return num_in_;
  }

  void dump(uint32_t* out) const {
    for (unsigned i = 0; i < 16; ++i) out[i] = state_[i];
    out[16] = num_in_;
    for (unsigned i = 0; i < 16; ++i) out[17 + i] = i < num_in_ ? in_[i] : 0;
    out[33] = num_out_;
    for (unsigned i = 0; i < 16; ++i) out[34 + i] = i < num_out_ ? out_[i] : 0;
  }

 private:
  void observe_one(uint32_t v) {
    num_out_ = 0;
    in_[num_in_++] = v;
    if (num_in_ == rate_) duplex();
  }

  void duplex() {
    for (unsigned i = 0; i < num_in_; ++i) state_[i] = in_[i];
    num_in_ = 0;
    poseidon2_bb::permute(external_, state_);
    for (unsigned i = 0; i < kChallengerWidth; ++i) out_[i] = state_[i];
    num_out_ = kChallengerWidth;
  }

  int external_;
  unsigned rate_;
  uint32_t state_[16] = {};
  uint32_t in_[16] = {};
  uint32_t out_[16] = {};
  unsigned num_in_ = 0, num_out_ = 0;
};

}  // namespace tachyon_amd::fri
