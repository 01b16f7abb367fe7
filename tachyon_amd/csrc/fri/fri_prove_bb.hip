// The queries of a FRI opening at many indices at once, and the whole opening
// proof in one call (see fri_bb.h):
//   queries_kernel   block (q, i) gathers query q's sibling value and digests
//                    of commit-phase tree i, over the folded vector of
//                    2^(log_max - i) elements; a single query is a batch of one
//   prove            TwoAdicFRI::CreateOpeningProof followed by fri::Prove
//                    (two_adic_fri.h:96-219, prove.h:121-159) in the
//                    reference's transcript order, with the grind on the GPU
//                    and one gather launch per tree for all queries
#include <algorithm>
#include <cstring>

#include "fri_bb.h"
#include "grind_bb.h"

namespace tachyon_amd::fri {

namespace {

constexpr unsigned kBlock = 256;
constexpr unsigned kMaxCommits = kMaxLogRows;
// queries_kernel gathers a tree's sibling digests with 8 lanes a digest in one block
static_assert(8 * (kMaxLogRows - 1) <= kBlock);

struct QueriesArgs {
  const Fp4* folded[kMaxCommits];
  const uint32_t* layers[kMaxCommits];
  uint32_t sib_off[kMaxCommits];  // digests of the trees before this one
  uint32_t log_max;
  uint32_t num_commits;
  uint32_t total_sibs;  // digests of one query
  const uint32_t* indices;
  uint32_t* vals;  // per query 4 words per tree
  uint32_t* sibs;  // per query 8 words per digest
};

__global__ __launch_bounds__(kBlock) void queries_kernel(const QueriesArgs a) {
  const uint32_t q = blockIdx.x, i = blockIdx.y, t = threadIdx.x;
  const uint32_t index_i = a.indices[q] >> i, pair = index_i >> 1;
  const uint32_t nsib = a.log_max - i - 1;  // the tree has 2^nsib leaves
  if (t < 4)
    a.vals[4 * ((size_t)q * a.num_commits + i) + t] = reinterpret_cast<const uint32_t*>(a.folded[i] + (index_i ^ 1))[t];
  hash::gather_siblings(a.layers[i], nsib, pair, a.sibs + 8 * ((size_t)q * a.total_sibs + a.sib_off[i]), t);
}

}  // namespace

bool FriOpening::answer_queries(const size_t* indices, size_t count, void* sibling_values_out, void* siblings_out) {
  if (!indices || !sibling_values_out || count == 0 || count > kMaxQueries) return false;
  for (size_t q = 0; q < count; ++q)
    if (!can_answer(phase_, indices[q])) return false;
  if (num_commits_ == 0) return true;  // nothing was committed: nothing to open
  const size_t total = query_total_siblings(phase_.log_max, (unsigned)num_commits_);
  if (total && !siblings_out) return false;
  const size_t idx_bytes = (count * sizeof(uint32_t) + 15) / 16 * 16;
  const size_t val_bytes = count * num_commits_ * sizeof(Fp4), sib_bytes = count * total * 8 * sizeof(uint32_t);
  std::vector<uint32_t> idx(idx_bytes / sizeof(uint32_t));
  for (size_t q = 0; q < count; ++q) idx[q] = (uint32_t)indices[q];
  uint8_t* d = static_cast<uint8_t*>(queries_.ensure(idx_bytes + val_bytes + sib_bytes));
  TA_HIP(hipMemcpyAsync(d, idx.data(), idx_bytes, hipMemcpyHostToDevice, stream_));
  QueriesArgs a{};
  uint32_t off = 0;
  for (size_t i = 0; i < num_commits_; ++i) {
    a.folded[i] = folded(i);
    a.layers[i] = trees_[i]->layers_device();
    a.sib_off[i] = off;
    off += query_num_siblings(phase_.log_max, (unsigned)i);
  }
  a.log_max = phase_.log_max;
  a.num_commits = (uint32_t)num_commits_;
  a.total_sibs = (uint32_t)total;
  a.indices = reinterpret_cast<const uint32_t*>(d);
  a.vals = reinterpret_cast<uint32_t*>(d + idx_bytes);
  a.sibs = reinterpret_cast<uint32_t*>(d + idx_bytes + val_bytes);
  hipLaunchKernelGGL(queries_kernel, dim3((unsigned)count, (unsigned)num_commits_), dim3(kBlock), 0, stream_, a);
  TA_HIP(hipGetLastError());
  launches_ = 1;
  TA_HIP(hipMemcpyAsync(sibling_values_out, a.vals, val_bytes, hipMemcpyDeviceToHost, stream_));
  if (total) TA_HIP(hipMemcpyAsync(siblings_out, a.sibs, sib_bytes, hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
  return true;
}

bool FriOpening::answer_query(size_t index, void* sibling_values_out, void* siblings_out) {
  // nothing was committed: nothing to open, whatever the outputs are
  if (num_commits_ == 0) return can_answer(phase_, index);
  return answer_queries(&index, 1, sibling_values_out, siblings_out);
}

bool FriOpening::prove(DuplexChallenger& challenger, const ProveRound* rounds, size_t num_rounds, size_t num_queries,
                       unsigned proof_of_work_bits, Proof* out) {
  if (!rounds || !out || num_rounds == 0 || num_queries == 0 || num_queries > kMaxQueries ||
      proof_of_work_bits > kMaxSampleBits || challenger.external() != external_)
    return false;
  // everything add_round would refuse is refused before begin() forgets the previous proof
  struct RoundArgs {
    std::vector<const void*> ldes;
    std::vector<size_t> rows, cols;
  };
  std::vector<RoundArgs> args(num_rounds);
  for (size_t r = 0; r < num_rounds; ++r) {
    const ProveRound& round = rounds[r];
    const hash::BbMerkleTree* tree = round.tree;
    if (!tree || !tree->built() || !(tree->flags() & merkle_tree::kFlagBitReversed) || tree->external() != external_)
      return false;
    const size_t count = tree->num_matrices();
    for (size_t m = 0; m < count; ++m) {
      args[r].ldes.push_back(tree->matrix(m));
      args[r].rows.push_back(tree->matrix_rows(m));
      args[r].cols.push_back(tree->matrix_cols(m));
    }
    if (!round_ok(args[r].ldes.data(), args[r].rows.data(), args[r].cols.data(), count, round.points,
                  round.num_points, round.opened_values_out, log_blowup_))
      return false;
    for (size_t m = 0; m < count; ++m)
      for (size_t p = 0; p < round.num_points[m]; ++p)
        for (int k = 0; k < 4; ++k)
          if (load_ext(round.points[m], p).c[k] >= bb31::kP) return false;
  }

  const DuplexChallenger at_entry = challenger;
  Proof proof;
  auto run = [&]() -> bool {
    Fp4 alpha;
    challenger.sample_ext(alpha.c);
    if (!begin(alpha)) return false;
    for (size_t r = 0; r < num_rounds; ++r)
      if (!add_round(args[r].ldes.data(), args[r].rows.data(), args[r].cols.data(), args[r].ldes.size(),
                     rounds[r].points, rounds[r].num_points, rounds[r].opened_values_out))
        return false;
    // CommitPhase: observe the root, sample beta, fold
    uint32_t root[8];
    int built;
    while ((built = commit(root)) == 1) {
      proof.commits.insert(proof.commits.end(), root, root + 8);
      challenger.observe(root, 8);
      Fp4 beta;
      challenger.sample_ext(beta.c);
      if (!fold(beta)) return false;
    }
    if (built != 0 || !ended(phase_)) return false;
    TA_HIP(hipMemcpyAsync(&proof.final_eval, folded(num_commits_), sizeof(Fp4), hipMemcpyDeviceToHost, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
    challenger.observe(proof.final_eval.c, 4);
    if (!grind(challenger, proof_of_work_bits, 0, bb31::kP, &proof.pow_witness, grind_, stream_)) return false;

    // every index is sampled after the witness: all queries are answered at once
    proof.log_max = phase_.log_max;
    proof.indices.resize(num_queries);
    for (size_t q = 0; q < num_queries; ++q) proof.indices[q] = challenger.sample_bits(phase_.log_max);
    const size_t total = query_total_siblings(phase_.log_max, (unsigned)num_commits_);
    proof.sibling_values.resize(std::max<size_t>(1, num_queries * num_commits_ * 4));
    proof.siblings.resize(std::max<size_t>(1, num_queries * total * 8));
    if (!answer_queries(proof.indices.data(), num_queries, proof.sibling_values.data(), proof.siblings.data()))
      return false;

    proof.rounds.resize(num_rounds);
    std::vector<size_t> shifted(num_queries);
    for (size_t r = 0; r < num_rounds; ++r) {
      hash::BbMerkleTree& tree = *rounds[r].tree;
      Proof::RoundOpenings& ro = proof.rounds[r];
      const unsigned log_round = tree.log_max();
      for (size_t q = 0; q < num_queries; ++q) shifted[q] = proof.indices[q] >> (phase_.log_max - log_round);
      ro.cols = args[r].cols;
      ro.num_siblings = log_round;
      ro.siblings.resize(std::max<size_t>(1, num_queries * log_round * 8));
      std::vector<void*> outs;
      for (size_t c : ro.cols) {
        ro.rows.emplace_back(num_queries * c);
        outs.push_back(ro.rows.back().data());
      }
      if (!tree.open_batch(shifted.data(), num_queries, outs.data(), ro.siblings.data())) return false;
    }
    return true;
  };
  bool ok = false;
  try {
    ok = run();
  } catch (...) {
    challenger = at_entry;
    throw;
  }
  if (!ok) {
    challenger = at_entry;
    return false;
  }
  *out = std::move(proof);
  return true;
}

}  // namespace tachyon_amd::fri
