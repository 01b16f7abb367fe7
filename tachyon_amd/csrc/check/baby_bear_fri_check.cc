// Exercise include/tachyon_mi355x_fri.h the way a Tachyon build runs
// TwoAdicFRI::Commit followed by CreateOpeningProof over BabyBear: Commit
// (CosetLDEBatch on the device and the bit-reversed build), then the opening on
// the extension where Commit left it, with a fixed alpha, one fixed point and
// fixed betas in place of a challenger.  Only the headers and the HIP runtime
// are used.
//   baby_bear_fri_check [--external horizen|plonky3] --gen <Montgomery word> <L> <cols> <queries>
//   --gen: the generator of order 2^(L + 1) as a Montgomery word (the caller
//          computes it; nothing comes from the library under test)
// The trace is 2^L x cols seeded words, log_blowup 1, shift 31.  alpha is the
// stored words {3, 1, 4, 1}, the point {5, 6, 7, 8}, beta of step i
// {i + 2, 3, 4, 5}; query q opens index (q * 2654435761) mod 2^(L + 1).
// Prints one JSON line with the commit root, the opened values, the
// commit-phase roots, the final values and the queries' sibling values and
// sibling digests for the caller to compare; exit 0 = every call returned true.
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
};

// seeded words in [0, p) (splitmix64, as baby_bear_merkle_check)
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

template <size_t N>
void print_words(const std::array<BabyBear, N>& a) {
  printf("[");
  for (size_t i = 0; i < N; ++i) printf("%s%u", i ? ", " : "", a[i].value);
  printf("]");
}

template <class T>
void print_list(const std::vector<T>& v) {
  printf("[");
  for (size_t i = 0; i < v.size(); ++i) {
    if (i) printf(", ");
    print_words(v[i]);
  }
  printf("]");
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
  if (!have_gen || numbers.size() != 3 || numbers[0] > 20 || numbers[1] == 0 || numbers[1] > 1024 ||
      numbers[2] > 64) {
    fprintf(stderr, "usage: baby_bear_fri_check [--external horizen|plonky3] --gen <Montgomery word> <L> <cols> <queries>\n");
    return 2;
  }
  const size_t rows = size_t(1) << numbers[0], cols = numbers[1], queries = numbers[2];
  const unsigned log_blowup = 1;
  const size_t out_rows = rows << log_blowup;
  const F shift_mont = {(uint32_t)((31ULL << 32) % kP)};

  auto icicle_ntt_holder_ = math::IcicleNTTHolder<F, math::kBabyBear>::Create();
  math::IcicleNTTOptions options;
  options.are_inputs_on_device = options.are_outputs_on_device = true;
  options.is_async = true;
  if (!icicle_ntt_holder_->Init(gen, options)) return 1;

  const std::vector<F> trace = seeded(0xF21F0000ULL, rows * cols);
  F* d_in = nullptr;
  F* d_lde = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_in), rows * cols * sizeof(F)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&d_lde), out_rows * cols * sizeof(F)) != hipSuccess ||
      hipMemcpy(d_in, trace.data(), rows * cols * sizeof(F), hipMemcpyHostToDevice) != hipSuccess)
    return 2;

  // Commit, then CreateOpeningProof on the same stream: no row of the extension leaves the device
  auto tree = crypto::Commit<F>(icicle_ntt_holder_, {{d_in, rows, cols}}, log_blowup, shift_mont, {d_lde}, external);
  if (!tree) return 1;
  const auto commitment = tree->GetRoot();

  Fri fri(log_blowup, external, icicle_ntt_holder_->stream());
  const ExtF alpha = {F{3}, F{1}, F{4}, F{1}}, zeta = {F{5}, F{6}, F{7}, F{8}};
  Fri::OpenedValuesForRound opened;
  bool ok = fri && fri.Begin(alpha) && fri.ReduceOpenings({{d_lde, out_rows, cols}}, {{zeta}}, &opened);
  std::vector<Fri::Digest> commits;
  uint32_t step = 0;
  ok = ok && fri.CommitPhase(
                 [&step](const Fri::Digest&) {
                   return ExtF{F{step++ + 2}, F{3}, F{4}, F{5}};
                 },
                 &commits);
  std::vector<std::vector<Fri::CommitPhaseProofStep>> answers(queries);
  std::vector<size_t> indices(queries);
  for (size_t q = 0; ok && q < queries; ++q) {
    indices[q] = (q * 2654435761ULL) % out_rows;
    ok = fri.AnswerQuery(indices[q], &answers[q]);
  }
  if (!ok) {
    printf("{\"calls\": false}\n");
    return 1;
  }

  printf("{\"calls\": true, \"commitment\": ");
  print_words(commitment);
  printf(", \"opened_values\": ");
  print_list(opened[0][0]);
  printf(", \"commit_phase_commits\": ");
  print_list(commits);
  printf(", \"final_poly\": ");
  print_list(fri.final_poly());
  printf(", \"queries\": [");
  for (size_t q = 0; q < queries; ++q) {
    printf("%s{\"index\": %zu, \"steps\": [", q ? ", " : "", indices[q]);
    for (size_t i = 0; i < answers[q].size(); ++i) {
      printf("%s{\"sibling_value\": ", i ? ", " : "");
      print_words(answers[q][i].sibling_value);
      printf(", \"opening_proof\": ");
      print_list(answers[q][i].opening_proof);
      printf("}");
    }
    printf("]}");
  }
  printf("]}\n");
  tree.reset();
  (void)hipFree(d_in);
  (void)hipFree(d_lde);
  return 0;
}
