// TwoAdicFRI::CreateOpeningProof over BabyBear / BabyBear4 on the GPU, all of
// it but the challenger (two_adic_fri.h, prove.h, fri_config.h): the reduced
// openings of every committed matrix, the commit phase (a FieldMerkleTree per
// fold step over the folded vector viewed as size/2 x 8 words) and the queries.
// alpha and each beta are inputs; each commit-phase root is handed back before
// the next beta is needed.  prove() runs the same steps with the transcript in
// a DuplexChallenger (challenger_bb.h), grinds on the GPU (grind_bb.h) and
// answers all queries at once (fri_prove_bb.hip).
//
// The matrices are the natural-order extensions Commit left on the coset
// 31 <w_n>.  The reference indexes everything in bit-reversed row order:
// position i is the natural row bitrev(i, log n) at x_i = 31 w_n^bitrev(i).
// Reduced openings, folded vectors and inverse denominators are kept in that
// order on the device, so a folded vector is its tree's leaf matrix as it
// stands, and the inverse denominators of a smaller height are a prefix of the
// largest one's.  No permuted copy of a matrix is made.
//
// Design constraints:
//  - a matrix's words are read from HBM 1 + 2^-log_blowup times per add_round:
//    every row once for rr[i] = sum_c alpha^c M[row(i)][c], the block of rows at
//    stride 2^log_blowup once for the interpolation, for up to kPointGroup
//    points.  Points are accumulated in registers; a matrix with more points
//    reads the block once per group of kPointGroup.
//  - (x - z)^-1 is computed once per point and largest height seen for it (a
//    later, taller matrix with the same point computes it again at that
//    height); its prefix of n >> log_blowup entries, negated, is the
//    interpolation's (z - x)^-1.
//  - rows are 4 cols bytes, so a lane per row would not coalesce: the rr pass
//    stages tiles of 256 positions x 32 columns through LDS with the lanes along
//    the columns, as merkle_bb.hip's hash_kernel does, and the interpolation
//    spreads its lanes over the columns.  Alpha powers come from a table made
//    once per begin(), through LDS, and the interpolation's per-row
//    coefficients from LDS too: nothing is recomputed per row and column.
//  - a zero denominator (a point inside 31 <w_n>, where the reference CHECKs)
//    sets a device flag; add_round returns false and the handle needs begin().
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../capi/fri_validate.h"
#include "../common/hip_util.h"
#include "../field/bb31x4.h"
#include "../hash/merkle_bb.h"
#include "challenger_bb.h"

namespace tachyon_amd::fri {

using bb31x4::Fp4;

inline constexpr unsigned kPointGroup = 8;     // points interpolated per read of the block

// The element at p[i] of a caller's array of 4-word elements, which is aligned
// to 4 bytes only (Fp4 is alignas(16)): copied, never reinterpreted.
inline Fp4 load_ext(const void* p, size_t i) {
  Fp4 v;
  memcpy(v.c, static_cast<const uint32_t*>(p) + 4 * i, sizeof v.c);
  return v;
}

enum Bb4Op : int { kBb4Add = 0, kBb4Sub = 1, kBb4Mul = 2, kBb4Square = 3, kBb4Inverse = 4, kBb4NumOps = 5 };

// out[i] = a[i] op b[i] on `count` elements of device memory (b unused by
// square and inverse), enqueued on `stream`
void bb4_ops(int op, const Fp4* d_a, const Fp4* d_b, Fp4* d_out, size_t count, hipStream_t stream);

// One commit round of FriOpening::prove: the round's tree (built with
// kFlagBitReversed over the natural-order extensions, which it still
// references) and add_round's points and outputs for the tree's matrices.
struct ProveRound {
  hash::BbMerkleTree* tree;
  const void* const* points;
  const size_t* num_points;
  void* const* opened_values_out;
};

// fri::FRIProof plus the input openings of TwoAdicFRI::CreateOpeningProof, in
// the layouts of answer_queries and BbMerkleTree::open_batch.
struct Proof {
  struct RoundOpenings {
    std::vector<size_t> cols;                 // per matrix
    std::vector<std::vector<uint32_t>> rows;  // per matrix: num_queries x cols words
    size_t num_siblings = 0;                  // digests per query
    std::vector<uint32_t> siblings;           // num_queries x num_siblings x 8 words
  };
  std::vector<uint32_t> commits;  // 8 words per commit-phase root
  Fp4 final_eval{};
  uint32_t pow_witness = 0;
  unsigned log_max = 0;
  std::vector<size_t> indices;
  std::vector<uint32_t> sibling_values;  // num_queries x num_commits x 4 words
  std::vector<uint32_t> siblings;        // num_queries x query_total_siblings x 8 words
  std::vector<RoundOpenings> rounds;
  size_t num_commits() const { return commits.size() / 8; }
};

class FriOpening {
 public:
  FriOpening(unsigned log_blowup, int external, hipStream_t stream);
  ~FriOpening();
  FriOpening(const FriOpening&) = delete;
  FriOpening& operator=(const FriOpening&) = delete;

  bool begin(const Fp4& alpha);
  // One round's matrices (host or device memory each; device matrices are
  // referenced and must stay alive until the reduced openings are no longer
  // needed, host matrices are uploaded).  points[m]: num_points[m] elements of
  // host memory; opened_values_out[m]: num_points[m] * cols[m] elements of host
  // memory, point-major.  Waits for the stream once.
  bool add_round(const void* const* ldes, const size_t* rows, const size_t* cols, size_t count,
                 const void* const* points, const size_t* num_points, void* const* opened_values_out);

  size_t num_inputs() const { return inputs_.size(); }
  unsigned input_log_size(size_t k) const { return k < inputs_.size() ? inputs_[k] : 0; }
  const Fp4* input_device(size_t k) const;
  bool input(size_t k, void* out);  // waits

  // 1: a tree over the folded vector was built and its root copied to root_out
  // (waits once); 0: the phase has ended; -1: refused
  int commit(void* root_out);
  bool fold(const Fp4& beta);
  size_t num_commits() const { return num_commits_; }
  bool final_poly(void* out);  // waits
  // answer_queries at one index, except that with no commit-phase tree the
  // outputs are not looked at.  Waits once.
  bool answer_query(size_t index, void* sibling_values_out, void* siblings_out);
  // The queries at `count` indices (fri_prove_bb.hip): per query, first array
  // 4 words per commit-phase tree, second 8 words per sibling digest, tree by
  // tree.  One launch, two copies, one wait.  False, with nothing written, for a
  // null pointer, count 0 or above kMaxQueries, or an index out of range.
  static constexpr size_t kMaxQueries = size_t(1) << 16;
  bool answer_queries(const size_t* indices, size_t count, void* sibling_values_out, void* siblings_out);

  // CreateOpeningProof followed by fri::Prove with the transcript in
  // `challenger` (fri_prove_bb.hip); see tachyon_mi355x_baby_bear_fri_opening_prove.
  // False with *out untouched on refusal; the challenger is then as it was, and
  // so is this opening unless a point lay inside the coset.
  bool prove(DuplexChallenger& challenger, const ProveRound* rounds, size_t num_rounds, size_t num_queries,
             unsigned proof_of_work_bits, Proof* out);

  unsigned log_blowup() const { return log_blowup_; }
  int external() const { return external_; }
  const Phase& phase() const { return phase_; }
  unsigned last_launches() const { return launches_; }
  hipStream_t stream() const { return stream_; }

 private:
  struct InvDenoms {
    Fp4 z;
    unsigned log_n;
    std::unique_ptr<DeviceBuffer> buf;
  };
  const Fp4* inv_denoms(const Fp4& z, unsigned log_n);
  void ensure_alpha_powers(size_t cols);
  const Fp4* folded(size_t i) const;  // the vector commit-phase tree i was built over

  unsigned log_blowup_;
  int external_;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  Phase phase_;
  Fp4 alpha_{};
  unsigned launches_ = 0;

  std::unique_ptr<DeviceBuffer> ro_[kMaxLogRows + 1];  // reduced openings by log height
  bool ro_present_[kMaxLogRows + 1] = {};
  size_t num_reduced_[kMaxLogRows + 1] = {};
  std::vector<unsigned> inputs_;  // log heights present, largest first

  std::vector<InvDenoms> inv_;
  std::vector<std::unique_ptr<DeviceBuffer>> uploads_;  // host matrices' device copies
  DeviceBuffer apow_;   // alpha^c, c < apow_count_
  size_t apow_count_ = 0;
  DeviceBuffer flag_;   // one word: a zero denominator was met
  DeviceBuffer pts_;    // the round's PointDev records
  DeviceBuffer ys_;     // the round's opened values
  DeviceBuffer partial_;  // the interpolation's per-row-block partial sums

  std::vector<std::unique_ptr<DeviceBuffer>> folds_;        // folds_[i]: the vector after fold step i + 1
  std::vector<std::unique_ptr<hash::BbMerkleTree>> trees_;  // trees_[i] over folded(i)
  size_t num_commits_ = 0;
  DeviceBuffer queries_;  // answer_queries: the indices, then the gathered answers
  DeviceBuffer grind_;    // prove: the grind's device word
};

}  // namespace tachyon_amd::fri
