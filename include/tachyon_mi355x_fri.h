/* The FRI opening over BabyBear / BabyBear4 on the MI355X: a header-only C++17
 * wrapper of the tachyon_mi355x_baby_bear_fri_opening_* C-ABI with the
 * reference's names (two_adic_fri.h:96-219, prove.h).  FriOpening::Prove is
 * TwoAdicFRI::CreateOpeningProof followed by fri::Prove in one call, with the
 * transcript in a DuplexChallenger and its Grind on the GPU.  The step-by-step
 * form stays: there the caller's transcript samples alpha, observes every
 * commit-phase root and samples the beta that follows it.
 *
 * F is the 4-byte BabyBear element (one uint32 Montgomery word); an extension
 * element is std::array<F, 4> (c0..c3 of F[x] / (x^4 - 11)).  The matrices are
 * the natural-order extensions Commit() of tachyon_mi355x_merkle_tree.h left
 * in the caller's ldes buffers. */
#ifndef TACHYON_MI355X_FRI_H_
#define TACHYON_MI355X_FRI_H_

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "tachyon_mi355x.h"
#include "tachyon_mi355x_merkle_tree.h"

namespace tachyon_mi355x {

enum class BabyBear4Op { kAdd = 0, kSub = 1, kMul = 2, kSquare = 3, kInverse = 4 };

/* out[i] = a[i] op b[i]; all host or all device memory (b unused by kSquare and
 * kInverse; the inverse of 0 is 0). */
template <class F>
[[nodiscard]] bool BabyBear4Ops(BabyBear4Op op, const std::array<F, 4>* a, const std::array<F, 4>* b,
                                std::array<F, 4>* out, size_t count, void* stream = nullptr) {
  static_assert(sizeof(F) == 4, "BabyBear: one uint32 Montgomery word");
  return tachyon_mi355x_baby_bear4_ops(static_cast<int>(op), a, b, out, count, stream) == 1;
}

/* DuplexChallenger<Poseidon2, 16, rate> over BabyBear (duplex_challenger.h,
 * challenger.h) on the host, with Grind on the GPU.  Copying clones the
 * transcript. */
template <class F>
class DuplexChallenger {
 public:
  static_assert(sizeof(F) == 4, "BabyBear: one uint32 Montgomery word");
  using ExtF = std::array<F, 4>;

  explicit DuplexChallenger(Poseidon2ExternalMatrix external = Poseidon2ExternalMatrix::kHorizen, uint32_t rate = 8)
      : handle_(tachyon_mi355x_baby_bear_duplex_challenger_create(static_cast<int>(external), rate)) {}
  DuplexChallenger(const DuplexChallenger& other)
      : handle_(tachyon_mi355x_baby_bear_duplex_challenger_clone(other.handle_)) {}
  DuplexChallenger& operator=(const DuplexChallenger& other) {
    if (this != &other) {
      tachyon_mi355x_baby_bear_duplex_challenger_destroy(handle_);
      handle_ = tachyon_mi355x_baby_bear_duplex_challenger_clone(other.handle_);
    }
    return *this;
  }
  ~DuplexChallenger() { tachyon_mi355x_baby_bear_duplex_challenger_destroy(handle_); }

  explicit operator bool() const { return handle_ != nullptr; }

  /* false, and nothing is observed, for a value that is not below p */
  [[nodiscard]] bool Observe(const F& value) { return ObserveWords(&value, 1); }
  template <class Container>
  [[nodiscard]] bool ObserveContainer(const Container& container) {
    return ObserveWords(container.data(), container.size());
  }

  F Sample() {
    F out{};
    if (handle_) (void)tachyon_mi355x_baby_bear_duplex_challenger_sample(handle_, reinterpret_cast<uint32_t*>(&out), 1);
    return out;
  }
  ExtF SampleExtElement() {
    ExtF out{};
    if (handle_) (void)tachyon_mi355x_baby_bear_duplex_challenger_sample_ext(handle_, out.data());
    return out;
  }
  /* bits <= 30 (the reference requires 2^bits < p); 0 without sampling above */
  uint32_t SampleBits(uint32_t bits) {
    uint32_t out = 0;
    if (handle_) (void)tachyon_mi355x_baby_bear_duplex_challenger_sample_bits(handle_, bits, &out);
    return out;
  }
  [[nodiscard]] bool CheckWitness(uint32_t bits, const F& witness) {
    uint32_t w;
    std::memcpy(&w, &witness, sizeof w);
    return handle_ && tachyon_mi355x_baby_bear_duplex_challenger_check_witness(handle_, bits, w) == 1;
  }
  /* Grind(bits) on the GPU: the smallest witness.  false (the reference
   * CHECKs) when there is none, with the transcript unchanged. */
  [[nodiscard]] bool Grind(uint32_t bits, F* witness, void* stream = nullptr) {
    return handle_ && witness &&
           tachyon_mi355x_baby_bear_duplex_challenger_grind(handle_, bits, reinterpret_cast<uint32_t*>(witness),
                                                            stream) == 1;
  }
  /* Grind(bits, Range) over the canonical candidates [from, to) */
  [[nodiscard]] bool Grind(uint32_t bits, uint32_t from, uint32_t to, F* witness, void* stream = nullptr) {
    return handle_ && witness &&
           tachyon_mi355x_baby_bear_duplex_challenger_grind_range(handle_, bits, from, to,
                                                                  reinterpret_cast<uint32_t*>(witness), stream) == 1;
  }

  tachyon_mi355x_baby_bear_duplex_challenger* handle() { return handle_; }

 private:
  bool ObserveWords(const F* values, size_t count) {
    return handle_ && tachyon_mi355x_baby_bear_duplex_challenger_observe(
                          handle_, reinterpret_cast<const uint32_t*>(values), count) == 1;
  }

  tachyon_mi355x_baby_bear_duplex_challenger* handle_ = nullptr;
};

template <class F>
class FriOpening {
 public:
  static_assert(sizeof(F) == 4, "BabyBear: one uint32 Montgomery word");
  using ExtF = std::array<F, 4>;
  using Digest = std::array<F, 8>;
  /* [matrix][point][column], OpenedValuesForRound of the reference */
  using OpenedValuesForRound = std::vector<std::vector<std::vector<ExtF>>>;
  struct CommitPhaseProofStep {
    ExtF sibling_value;
    std::vector<Digest> opening_proof;
  };

  explicit FriOpening(uint32_t log_blowup, Poseidon2ExternalMatrix external = Poseidon2ExternalMatrix::kHorizen,
                      void* stream = nullptr)
      : handle_(tachyon_mi355x_baby_bear_fri_opening_create(log_blowup, static_cast<int>(external), stream)),
        log_blowup_(log_blowup) {}
  FriOpening(const FriOpening&) = delete;
  FriOpening& operator=(const FriOpening&) = delete;
  ~FriOpening() { tachyon_mi355x_baby_bear_fri_opening_destroy(handle_); }

  explicit operator bool() const { return handle_ != nullptr; }

  /* Forgets the previous proof and sets the batching challenge. */
  [[nodiscard]] bool Begin(const ExtF& alpha) {
    return handle_ && tachyon_mi355x_baby_bear_fri_opening_begin(handle_, alpha.data()) == 1;
  }

  /* One commit round of CreateOpeningProof's first half: the opened values of
   * every matrix at its points, and the round's share of the reduced openings
   * (kept on the device).  Call once per round, in the rounds' order.  Device
   * matrices are referenced until the next Begin().  false on refusal (see
   * tachyon_mi355x.h); after a point inside the committed coset the opening
   * needs a new Begin(). */
  [[nodiscard]] bool ReduceOpenings(const std::vector<MatrixView<F>>& ldes,
                                    const std::vector<std::vector<ExtF>>& points,
                                    OpenedValuesForRound* opened_values) {
    if (!handle_ || !opened_values || points.size() != ldes.size()) return false;
    const size_t n = ldes.size();
    std::vector<const void*> data(n);
    std::vector<size_t> rows(n), cols(n);
    for (size_t m = 0; m < n; ++m) {
      data[m] = ldes[m].data;
      rows[m] = ldes[m].rows;
      cols[m] = ldes[m].cols;
    }
    PointArgs args(points, cols);
    if (tachyon_mi355x_baby_bear_fri_opening_add_round(handle_, data.data(), rows.data(), cols.data(), n,
                                                       args.points.data(), args.num.data(), args.out.data()) != 1)
      return false;
    *opened_values = args.Opened();
    return true;
  }

  size_t num_inputs() const { return handle_ ? tachyon_mi355x_baby_bear_fri_opening_num_inputs(handle_) : 0; }
  uint32_t input_log_size(size_t k) const {
    return handle_ ? tachyon_mi355x_baby_bear_fri_opening_input_log_size(handle_, k) : 0;
  }
  /* reduced opening k, largest first, in the reference's bit-reversed order */
  std::vector<ExtF> input(size_t k) const {
    if (k >= num_inputs()) return {};
    std::vector<ExtF> v(size_t{1} << input_log_size(k));
    if (tachyon_mi355x_baby_bear_fri_opening_input(handle_, k, v.data()) != 1) return {};
    return v;
  }
  const ExtF* input_device(size_t k) const {
    return handle_ ? static_cast<const ExtF*>(tachyon_mi355x_baby_bear_fri_opening_input_device_ptr(handle_, k))
                   : nullptr;
  }

  /* fri::CommitPhase: on_commit(const Digest&) -> ExtF is the caller's
   * challenger.ObserveContainer(commit) followed by SampleExtElement.  The
   * commitments are appended to *commits.  false when nothing was reduced. */
  template <class OnCommit>
  [[nodiscard]] bool CommitPhase(OnCommit&& on_commit, std::vector<Digest>* commits) {
    if (!handle_ || !commits || num_inputs() == 0) return false;
    Digest root;
    while (tachyon_mi355x_baby_bear_fri_opening_commit(handle_, root.data()) == 1) {
      commits->push_back(root);
      const ExtF beta = on_commit(static_cast<const Digest&>(root));
      if (tachyon_mi355x_baby_bear_fri_opening_fold(handle_, beta.data()) != 1) return false;
    }
    std::vector<ExtF> poly(size_t{1} << log_blowup_);
    if (tachyon_mi355x_baby_bear_fri_opening_final_poly(handle_, poly.data()) != 1) return false;
    final_poly_ = std::move(poly);
    return true;
  }

  size_t num_commits() const { return handle_ ? tachyon_mi355x_baby_bear_fri_opening_num_commits(handle_) : 0; }
  /* the last 2^log_blowup values (all equal for honest inputs), after CommitPhase */
  const std::vector<ExtF>& final_poly() const { return final_poly_; }
  ExtF final_eval() const { return final_poly_.empty() ? ExtF{} : final_poly_[0]; }

  /* fri::AnswerQuery: one step per commit-phase tree.  The input openings are
   * the caller's CreateOpeningProof(index >> bits_reduced) on the round trees. */
  [[nodiscard]] bool AnswerQuery(size_t index, std::vector<CommitPhaseProofStep>* steps) const {
    if (!handle_ || !steps || num_inputs() == 0) return false;
    const size_t commits = num_commits();
    const uint32_t log_max = input_log_size(0);
    std::vector<ExtF> values(commits + 1);
    std::vector<Digest> siblings(TotalSiblings(log_max, commits) + 1);
    if (tachyon_mi355x_baby_bear_fri_opening_answer_query(handle_, index, values.data(), siblings.data()) != 1)
      return false;
    *steps = SplitSteps(values.data(), siblings.data(), log_max, commits);
    return true;
  }

  /* fri::AnswerQuery at every index with one launch */
  [[nodiscard]] bool AnswerQueries(const std::vector<size_t>& indices,
                                   std::vector<std::vector<CommitPhaseProofStep>>* steps) const {
    if (!handle_ || !steps || num_inputs() == 0) return false;
    const size_t commits = num_commits(), count = indices.size();
    const uint32_t log_max = input_log_size(0);
    const size_t total = TotalSiblings(log_max, commits);
    std::vector<ExtF> values(count * commits + 1);
    std::vector<Digest> siblings(count * total + 1);
    if (tachyon_mi355x_baby_bear_fri_opening_answer_queries(handle_, indices.data(), count, values.data(),
                                                            siblings.data()) != 1)
      return false;
    steps->clear();
    for (size_t q = 0; q < count; ++q)
      steps->push_back(SplitSteps(values.data() + q * commits, siblings.data() + q * total, log_max, commits));
    return true;
  }

  /* The reference's proof types (fri_proof.h, two_adic_fri.h). */
  struct BatchOpening {
    std::vector<std::vector<F>> opened_values;  /* the opened row per matrix of the round */
    std::vector<Digest> opening_proof;
  };
  struct QueryProof {
    std::vector<BatchOpening> input_proof;  /* one per round */
    std::vector<CommitPhaseProofStep> commit_phase_openings;
  };
  struct FRIProof {
    std::vector<Digest> commit_phase_commits;
    std::vector<QueryProof> query_proofs;
    ExtF final_eval{};
    F pow_witness{};
    std::vector<size_t> query_indices;  /* what the verifier samples again */
  };
  /* One commit round: the tree Commit() returned and the opening points of
   * each of its matrices. */
  struct Round {
    FieldMerkleTree<F>* tree = nullptr;
    std::vector<std::vector<ExtF>> points;
  };

  /* TwoAdicFRI::CreateOpeningProof followed by fri::Prove in one call, the
   * transcript in `challenger` (which has observed what precedes alpha).  The
   * opened values are returned for the caller to observe afterwards, as in the
   * reference.  false on refusal (see tachyon_mi355x.h), with the challenger
   * as it was. */
  [[nodiscard]] bool Prove(DuplexChallenger<F>& challenger, const std::vector<Round>& rounds, size_t num_queries,
                           uint32_t proof_of_work_bits, FRIProof* proof,
                           std::vector<OpenedValuesForRound>* opened_values) {
    if (!handle_ || !challenger || !proof || !opened_values || rounds.empty()) return false;
    const size_t nr = rounds.size();
    std::vector<tachyon_mi355x_baby_bear_fri_round> recs(nr);
    std::vector<PointArgs> args;
    args.reserve(nr);
    for (size_t r = 0; r < nr; ++r) {
      const Round& round = rounds[r];
      if (!round.tree || round.points.size() != round.tree->leaves().size()) return false;
      std::vector<size_t> cols;
      for (const auto& leaf : round.tree->leaves()) cols.push_back(leaf.cols);
      args.emplace_back(round.points, cols);
      recs[r] = {round.tree->handle(), args[r].points.data(), args[r].num.data(), args[r].out.data()};
    }
    tachyon_mi355x_baby_bear_fri_proof* p = tachyon_mi355x_baby_bear_fri_opening_prove(
        handle_, challenger.handle(), recs.data(), nr, num_queries, proof_of_work_bits);
    if (!p) return false;

    std::vector<OpenedValuesForRound> opened;
    for (const PointArgs& a : args) opened.push_back(a.Opened());
    FRIProof result;
    const size_t commits = tachyon_mi355x_baby_bear_fri_proof_num_commits(p);
    const uint32_t log_max = input_log_size(0);
    result.commit_phase_commits.resize(commits);
    Digest unused;
    bool ok = tachyon_mi355x_baby_bear_fri_proof_commits(
                  p, commits ? result.commit_phase_commits.data()->data() : unused.data()) == 1 &&
              tachyon_mi355x_baby_bear_fri_proof_final_eval(p, result.final_eval.data()) == 1 &&
              tachyon_mi355x_baby_bear_fri_proof_pow_witness(p, reinterpret_cast<uint32_t*>(&result.pow_witness)) == 1;
    const size_t queries = tachyon_mi355x_baby_bear_fri_proof_num_queries(p);
    result.query_proofs.resize(queries);
    std::vector<ExtF> values(commits + 1);
    std::vector<Digest> siblings(TotalSiblings(log_max, commits) + 1);
    for (size_t q = 0; ok && q < queries; ++q) {
      QueryProof& qp = result.query_proofs[q];
      result.query_indices.push_back(tachyon_mi355x_baby_bear_fri_proof_query_index(p, q));
      ok = tachyon_mi355x_baby_bear_fri_proof_query_steps(p, q, values.data(), siblings.data()) == 1;
      if (ok) qp.commit_phase_openings = SplitSteps(values.data(), siblings.data(), log_max, commits);
      for (size_t r = 0; ok && r < nr; ++r) {
        const auto& leaves = rounds[r].tree->leaves();
        BatchOpening opening;
        std::vector<void*> rows(leaves.size());
        for (size_t m = 0; m < leaves.size(); ++m) {
          opening.opened_values.emplace_back(leaves[m].cols);
          rows[m] = opening.opened_values.back().data();
        }
        const size_t layers = tachyon_mi355x_baby_bear_merkle_tree_num_layers(rounds[r].tree->handle());
        opening.opening_proof.resize(layers - 1);
        ok = tachyon_mi355x_baby_bear_fri_proof_query_input(
                 p, q, r, rows.data(), layers > 1 ? opening.opening_proof.data()->data() : unused.data()) == 1;
        qp.input_proof.push_back(std::move(opening));
      }
    }
    tachyon_mi355x_baby_bear_fri_proof_destroy(p);
    if (!ok) return false;
    *proof = std::move(result);
    *opened_values = std::move(opened);
    return true;
  }

  unsigned last_launches() const { return handle_ ? tachyon_mi355x_baby_bear_fri_opening_last_launches(handle_) : 0; }
  void* stream() const { return handle_ ? tachyon_mi355x_baby_bear_fri_opening_stream(handle_) : nullptr; }
  tachyon_mi355x_baby_bear_fri_opening* handle() { return handle_; }

 private:
  /* digests of all commit-phase openings of one query */
  static size_t TotalSiblings(uint32_t log_max, size_t commits) {
    size_t total = 0;
    for (size_t i = 0; i < commits; ++i) total += log_max - i - 1;
    return total;
  }

  /* one query's steps from its sibling values and its digests, tree by tree */
  static std::vector<CommitPhaseProofStep> SplitSteps(const ExtF* values, const Digest* siblings, uint32_t log_max,
                                                      size_t commits) {
    std::vector<CommitPhaseProofStep> steps;
    for (size_t i = 0; i < commits; ++i) {
      const size_t n = log_max - i - 1;
      steps.push_back({values[i], std::vector<Digest>(siblings, siblings + n)});
      siblings += n;
    }
    return steps;
  }

  /* add_round's points, num_points and opened_values_out for one round's
   * matrices of `cols` columns, and the opened values the call left in them.
   * `pts` is referenced, not copied. */
  struct PointArgs {
    PointArgs(const std::vector<std::vector<ExtF>>& pts, const std::vector<size_t>& cols) : cols(cols) {
      for (size_t m = 0; m < cols.size(); ++m) {
        points.push_back(pts[m].data());
        num.push_back(pts[m].size());
        flat.emplace_back(pts[m].size() * cols[m]);
      }
      for (auto& f : flat) out.push_back(f.data());
    }
    OpenedValuesForRound Opened() const {
      OpenedValuesForRound result(cols.size());
      for (size_t m = 0; m < cols.size(); ++m)
        for (size_t p = 0; p < num[m]; ++p)
          result[m].emplace_back(flat[m].begin() + p * cols[m], flat[m].begin() + (p + 1) * cols[m]);
      return result;
    }
    std::vector<size_t> cols, num;
    std::vector<const void*> points;
    std::vector<void*> out;
    std::vector<std::vector<ExtF>> flat;
  };

  tachyon_mi355x_baby_bear_fri_opening* handle_ = nullptr;
  uint32_t log_blowup_ = 0;
  std::vector<ExtF> final_poly_;
};

}  // namespace tachyon_mi355x

#endif  // TACHYON_MI355X_FRI_H_
