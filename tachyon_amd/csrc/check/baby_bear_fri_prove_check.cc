// Exercise include/tachyon_mi355x_fri.h's one-call opening the way a Tachyon
// build runs TwoAdicFRI::Commit, CreateOpeningProof and fri::Prove over
// BabyBear: Commit (CosetLDEBatch on the device and the bit-reversed build),
// then FriOpening::Prove with a DuplexChallenger as the transcript.  Only the
// headers and the HIP runtime are used.
//   baby_bear_fri_prove_check [--external horizen|plonky3] --gen <Montgomery word> <L> <cols> <queries> <bits>
//   --gen: the generator of order 2^(L + 1) as a Montgomery word (the caller
//          computes it; nothing comes from the library under test)
// The trace is 2^L x cols seeded words, log_blowup 1, shift 31.  The proof is
// then checked against the step-by-step API on a second opening, driven by a
// second challenger that replays the transcript: the same alpha and betas, the
// same roots and final value, CheckWitness accepts the witness, SampleBits
// gives the proof's indices, and AnswerQuery / CreateOpeningProof at each index
// give the proof's openings.  Prints one JSON line; exit 0 = everything agreed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../../include/tachyon_mi355x_fri.h"

namespace {

constexpr uint32_t kP = 0x78000001u;

struct BabyBear {
  uint32_t value;
  bool operator==(const BabyBear& o) const { return value == o.value; }
};

// seeded words in [0, p) (splitmix64, as baby_bear_fri_check)
std::vector<BabyBear> seeded(uint64_t seed, size_t n) {
  std::vector<BabyBear> v(n);
  uint64_t x = seed;
  for (size_t i = 0; i < n; ++i) {
    x += 0x9e3779b97f4a7c15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    v[i].value = (uint32_t)(z % kP);
  }
  return v;
}

int fail(const char* what) {
  printf("{\"ok\": false, \"failed\": \"%s\"}\n", what);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  namespace crypto = tachyon_mi355x;
  namespace math = tachyon_mi355x;
  using F = BabyBear;
  using Fri = crypto::FriOpening<F>;
  using ExtF = Fri::ExtF;
  crypto::Poseidon2ExternalMatrix external = crypto::Poseidon2ExternalMatrix::kHorizen;
  bool have_gen = false;
  F gen = {0};
  std::vector<size_t> numbers;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--gen" && i + 1 < argc) gen.value = (uint32_t)strtoul(argv[++i], nullptr, 10), have_gen = true;
    else if (a == "--external" && i + 1 < argc && std::string(argv[i + 1]) == "horizen") ++i;
    else if (a == "--external" && i + 1 < argc && std::string(argv[i + 1]) == "plonky3")
      external = crypto::Poseidon2ExternalMatrix::kPlonky3, ++i;
    else numbers.push_back(strtoul(a.c_str(), nullptr, 10));
  }
  if (!have_gen || numbers.size() != 4 || numbers[0] > 20 || numbers[1] == 0 || numbers[1] > 1024 ||
      numbers[2] == 0 || numbers[2] > 256 || numbers[3] > 20) {
    fprintf(stderr,
            "usage: baby_bear_fri_prove_check [--external horizen|plonky3] --gen <Montgomery word> <L> <cols> "
            "<queries> <bits>\n");
    return 2;
  }
  const size_t rows = size_t(1) << numbers[0], cols = numbers[1], queries = numbers[2];
  const uint32_t bits = (uint32_t)numbers[3];
  const unsigned log_blowup = 1;
  const size_t out_rows = rows << log_blowup;
  const F shift_mont = {(uint32_t)((31ULL << 32) % kP)};

  auto icicle_ntt_holder_ = math::IcicleNTTHolder<F, math::kBabyBear>::Create();
  math::IcicleNTTOptions options;
  options.are_inputs_on_device = options.are_outputs_on_device = true;
  options.is_async = true;
  if (!icicle_ntt_holder_->Init(gen, options)) return fail("Init");

  const std::vector<F> trace = seeded(0xF21F0001ULL, rows * cols);
  F* d_in = nullptr;
  F* d_lde = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_in), rows * cols * sizeof(F)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&d_lde), out_rows * cols * sizeof(F)) != hipSuccess ||
      hipMemcpy(d_in, trace.data(), rows * cols * sizeof(F), hipMemcpyHostToDevice) != hipSuccess)
    return 2;

  auto tree = crypto::Commit<F>(icicle_ntt_holder_, {{d_in, rows, cols}}, log_blowup, shift_mont, {d_lde}, external);
  if (!tree) return fail("Commit");
  const auto commitment = tree->GetRoot();

  // the transcript: the commitment, zeta, then everything Prove does
  crypto::DuplexChallenger<F> challenger(external);
  if (!challenger || !challenger.ObserveContainer(commitment)) return fail("ObserveContainer");
  const ExtF zeta = challenger.SampleExtElement();
  crypto::DuplexChallenger<F> replay = challenger;  // the copy constructor clones

  Fri fri(log_blowup, external, icicle_ntt_holder_->stream());
  Fri::FRIProof proof;
  std::vector<Fri::OpenedValuesForRound> opened;
  if (!fri || !fri.Prove(challenger, {{tree.get(), {{zeta}}}}, queries, bits, &proof, &opened)) return fail("Prove");
  if (proof.query_proofs.size() != queries || opened.size() != 1 || opened[0][0][0].size() != cols)
    return fail("shape");

  // the step-by-step API on a second opening, driven by the replayed transcript
  Fri steps(log_blowup, external, icicle_ntt_holder_->stream());
  Fri::OpenedValuesForRound step_opened;
  const ExtF alpha = replay.SampleExtElement();
  if (!steps || !steps.Begin(alpha) || !steps.ReduceOpenings({{d_lde, out_rows, cols}}, {{zeta}}, &step_opened))
    return fail("ReduceOpenings");
  if (!(step_opened == opened[0])) return fail("opened values differ");
  std::vector<Fri::Digest> commits;
  bool observed = true;
  if (!steps.CommitPhase(
          [&](const Fri::Digest& root) {
            observed = observed && replay.ObserveContainer(root);
            return replay.SampleExtElement();
          },
          &commits) ||
      !observed)
    return fail("CommitPhase");
  if (!(commits == proof.commit_phase_commits)) return fail("commit_phase_commits differ");
  if (!(steps.final_eval() == proof.final_eval)) return fail("final_eval differs");
  if (!replay.ObserveContainer(proof.final_eval)) return fail("observe final_eval");
  if (!replay.CheckWitness(bits, proof.pow_witness)) return fail("CheckWitness");
  const uint32_t log_max = steps.input_log_size(0);
  for (size_t q = 0; q < queries; ++q) {
    const size_t index = replay.SampleBits(log_max);
    if (index != proof.query_indices[q]) return fail("query index differs");
    std::vector<Fri::CommitPhaseProofStep> answer;
    if (!steps.AnswerQuery(index, &answer)) return fail("AnswerQuery");
    const auto& got = proof.query_proofs[q].commit_phase_openings;
    if (answer.size() != got.size()) return fail("steps differ");
    for (size_t i = 0; i < answer.size(); ++i)
      if (!(answer[i].sibling_value == got[i].sibling_value) || !(answer[i].opening_proof == got[i].opening_proof))
        return fail("commit_phase_openings differ");
    std::vector<std::vector<F>> rows_opened;
    std::vector<Fri::Digest> siblings;
    if (!tree->CreateOpeningProof(index, &rows_opened, &siblings)) return fail("CreateOpeningProof");
    const auto& input = proof.query_proofs[q].input_proof;
    if (input.size() != 1 || !(input[0].opened_values == rows_opened) || !(input[0].opening_proof == siblings))
      return fail("input_proof differs");
  }
  // the transcript can go on from either challenger
  if (!(challenger.Sample() == replay.Sample())) return fail("transcripts diverge");

  printf("{\"ok\": true, \"commits\": %zu, \"queries\": %zu, \"pow_witness\": %u}\n", proof.commit_phase_commits.size(),
         queries, proof.pow_witness.value);
  tree.reset();
  (void)hipFree(d_in);
  (void)hipFree(d_lde);
  return 0;
}
