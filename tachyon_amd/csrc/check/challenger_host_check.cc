// The Poseidon2 and DuplexChallenger headers on the host, on their own, with a plain
// host compiler and no library: the known answers of tests/test_challenger.py
// walked in C++, so that the headers can be run under the host sanitizers
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       check/challenger_host_check.cc -o challenger_host_check && ./challenger_host_check
// Exit 0 = every answer matched.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../fri/challenger_bb.h"

namespace {

using namespace tachyon_amd;

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

bool equal_canonical(const uint32_t* mont, const uint32_t* want, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (bb31::from_mont(mont[i]) != want[i]) return false;
  return true;
}

}  // namespace

int main() {
  namespace host = poseidon2_bb;

  // Poseidon2 of 0..15 (Horizen) and of 16 times p - 1: tests/golden/poseidon2_baby_bear.json
  const uint32_t horizen_0_to_15[16] = {1699737005, 296394369,  268410240, 828329642, 1491697358, 1128780676,
                                        287184043,  1806152977, 1380147856, 345666717, 491196631,  1875224538,
                                        697740550,  1854502887, 1201727753, 1802410886};
  const uint32_t horizen_pm1[16] = {1035701041, 1597888870, 1069472689, 1384861682, 1704759606, 907480256,
                                    1081318776, 17038809,   966349349,  584280797,  1688185620, 945842140,
                                    1544649776, 1760104941, 21512725,   1575095462};
  uint32_t s[16];
  for (uint32_t i = 0; i < 16; ++i) s[i] = bb31::to_mont(i);
  host::permute(host::kHorizen, s);
  expect(equal_canonical(s, horizen_0_to_15, 16), "Horizen permutation of 0..15");
  for (uint32_t i = 0; i < 16; ++i) s[i] = bb31::to_mont(bb31::kP - 1);
  host::permute(host::kHorizen, s);
  expect(equal_canonical(s, horizen_pm1, 16), "Horizen permutation of 16 x (p - 1)");

  // duplex_challenger_unittest.cc:44-56: Plonky3, rate 4, observe 0..19, 10 samples
  const uint32_t samples[10] = {1091695522, 747772208, 1145639564, 1789312616, 567623980,
                                179016966,  125050365, 1725901131, 65962335,  1086560956};
  fri::DuplexChallenger ch(host::kPlonky3, 4);
  std::vector<uint32_t> values(20);
  for (uint32_t i = 0; i < 20; ++i) values[i] = bb31::to_mont(i);
  expect(ch.observe(values.data(), values.size()), "observe 0..19");
  expect(ch.num_inputs() == 0 && ch.num_outputs() == 16, "a full buffer is duplexed at once");
  uint32_t got[10];
  for (int i = 0; i < 10; ++i) got[i] = ch.sample();
  expect(equal_canonical(got, samples, 10), "the reference's 10 samples");

  // every rate, buffers at their limits: observe rate - 1 words, sample 17 times, clone, dump
  for (unsigned rate = 1; rate <= 16; ++rate) {
    fri::DuplexChallenger c(host::kHorizen, rate);
    expect(c.observe(values.data(), rate - 1), "partial observe");
    expect(c.num_inputs() == (rate == 1 ? 0 : rate - 1), "input buffer length");
    for (int i = 0; i < 17; ++i) (void)c.sample();
    expect(c.num_outputs() == 15, "the output buffer is refilled when it runs out");
    fri::DuplexChallenger twin = c;
    const uint32_t w = bb31::to_mont(7);
    expect(c.check_witness(4, w) == twin.check_witness(4, w), "a clone follows the same transcript");
    uint32_t base[16], dump[fri::kChallengerStateWords];
    expect(c.grind_base(base) == c.num_inputs(), "grind slot");
    c.dump(dump);
    expect(dump[16] == c.num_inputs() && dump[33] == c.num_outputs(), "dump lengths");
    (void)c.sample_bits(0);
    (void)c.sample_bits(30);
    uint32_t e[4];
    c.sample_ext(e);
  }

  // a non-canonical word: nothing is observed
  fri::DuplexChallenger r(host::kHorizen, 8);
  const uint32_t bad[3] = {1, 2, bb31::kP};
  expect(!r.observe(bad, 3) && r.num_inputs() == 0, "a word >= p is refused");
  expect(!fri::challenger_rate_ok(0) && !fri::challenger_rate_ok(17) && fri::challenger_rate_ok(16), "rates");

  if (failures == 0) printf("challenger_host_check ok\n");
  return failures == 0 ? 0 : 1;
}
