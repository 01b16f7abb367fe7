/* The FRI opening over BabyBear / BabyBear4 on the MI355X: a header-only C++17
 * wrapper of the tachyon_mi355x_baby_bear_fri_opening_* C-ABI with the
 * reference's names (two_adic_fri.h:96-219, prove.h).  It is
 * TwoAdicFRI::CreateOpeningProof without the challenger: the caller's
 * transcript samples alpha, observes every commit-phase root and samples the
 * beta that follows it.
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
    std::vector<const void*> data(n), pts(n);
    std::vector<void*> out(n);
    std::vector<size_t> rows(n), cols(n), num(n);
    std::vector<std::vector<ExtF>> flat(n);
    for (size_t m = 0; m < n; ++m) {
      data[m] = ldes[m].data;
      rows[m] = ldes[m].rows;
      cols[m] = ldes[m].cols;
      num[m] = points[m].size();
      pts[m] = points[m].data();
      flat[m].resize(points[m].size() * ldes[m].cols);
      out[m] = flat[m].data();
    }
    if (tachyon_mi355x_baby_bear_fri_opening_add_round(handle_, data.data(), rows.data(), cols.data(), n, pts.data(),
                                                       num.data(), out.data()) != 1)
      return false;
    OpenedValuesForRound result(n);
    for (size_t m = 0; m < n; ++m)
      for (size_t p = 0; p < points[m].size(); ++p)
        result[m].emplace_back(flat[m].begin() + p * cols[m], flat[m].begin() + (p + 1) * cols[m]);
    *opened_values = std::move(result);
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
    size_t total = 0;
    for (size_t i = 0; i < commits; ++i) total += log_max - i - 1;
    std::vector<ExtF> values(commits + 1);
    std::vector<Digest> siblings(total + 1);
    if (tachyon_mi355x_baby_bear_fri_opening_answer_query(handle_, index, values.data(), siblings.data()) != 1)
      return false;
    steps->clear();
    size_t at = 0;
    for (size_t i = 0; i < commits; ++i) {
      const size_t count = log_max - i - 1;
      steps->push_back({values[i], std::vector<Digest>(siblings.begin() + at, siblings.begin() + at + count)});
      at += count;
    }
    return true;
  }

  unsigned last_launches() const { return handle_ ? tachyon_mi355x_baby_bear_fri_opening_last_launches(handle_) : 0; }
  void* stream() const { return handle_ ? tachyon_mi355x_baby_bear_fri_opening_stream(handle_) : nullptr; }
  tachyon_mi355x_baby_bear_fri_opening* handle() { return handle_; }

 private:
  tachyon_mi355x_baby_bear_fri_opening* handle_ = nullptr;
  uint32_t log_blowup_ = 0;
  std::vector<ExtF> final_poly_;
};

}  // namespace tachyon_mi355x

#endif  // TACHYON_MI355X_FRI_H_
