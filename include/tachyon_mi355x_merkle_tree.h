/* FieldMerkleTree<BabyBear, 8> and the commit step of TwoAdicFRI on the MI355X:
 * a header-only C++17 wrapper of the tachyon_mi355x_baby_bear_merkle_tree_*
 * C-ABI with the reference's member names (field_merkle_tree.h,
 * field_merkle_tree_mmcs.h, two_adic_fri.h:76-94).
 *
 * F is the 4-byte BabyBear element (one uint32 Montgomery word).  The hashers
 * are fixed to the configuration the reference uses: Poseidon2 of width 16,
 * PaddingFreeSponge<., 8, 8>, TruncatedPermutation<., 8, 2>; the external
 * matrix (Horizen or Plonky3) is chosen at construction.  A BabyBear4 matrix is
 * passed as the base-field matrix with 4 x the columns. */
#ifndef TACHYON_MI355X_MERKLE_TREE_H_
#define TACHYON_MI355X_MERKLE_TREE_H_

#include <array>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "tachyon_mi355x.h"
#include "tachyon_mi355x_ntt_holder.h"

namespace tachyon_mi355x {

enum class Poseidon2ExternalMatrix { kHorizen = TACHYON_MI355X_POSEIDON2_HORIZEN, kPlonky3 = TACHYON_MI355X_POSEIDON2_PLONKY3 };

/* Poseidon2Sponge::Permute on `count` states of 16 elements, host or device
 * memory, in place. */
template <class F>
[[nodiscard]] bool Poseidon2Permute(Poseidon2ExternalMatrix external, F* states, size_t count,
                                    void* stream = nullptr) {
  static_assert(sizeof(F) == 4, "BabyBear: one uint32 Montgomery word");
  return tachyon_mi355x_poseidon2_baby_bear_permute(static_cast<int>(external), states, count, stream) == 1;
}

/* A row-major matrix view, host or device memory (Eigen::Map<const
 * RowMajorMatrix<F>> in the reference). */
template <class F>
struct MatrixView {
  const F* data = nullptr;
  size_t rows = 0;
  size_t cols = 0;
};

template <class F>
class FieldMerkleTree {
 public:
  static_assert(sizeof(F) == 4, "BabyBear: one uint32 Montgomery word");
  using Digest = std::array<F, 8>;

  explicit FieldMerkleTree(Poseidon2ExternalMatrix external = Poseidon2ExternalMatrix::kHorizen,
                           void* stream = nullptr)
      : handle_(tachyon_mi355x_baby_bear_merkle_tree_create(static_cast<int>(external), stream)) {}
  FieldMerkleTree(const FieldMerkleTree&) = delete;
  FieldMerkleTree& operator=(const FieldMerkleTree&) = delete;
  FieldMerkleTree(FieldMerkleTree&& other) noexcept
      : handle_(other.handle_), leaves_(std::move(other.leaves_)), bit_reversed_(other.bit_reversed_) {
    other.handle_ = nullptr;
  }
  ~FieldMerkleTree() { tachyon_mi355x_baby_bear_merkle_tree_destroy(handle_); }

  /* FieldMerkleTree::Build.  Device matrices are referenced, not copied: they
   * stay alive for CreateOpeningProof.  bit_reversed: leaf i of a matrix is its
   * stored row bitrev(i); every height must then be a power of two.  false on
   * refusal (see tachyon_mi355x.h), the tree keeping what it held. */
  [[nodiscard]] bool Build(const std::vector<MatrixView<F>>& leaves, bool bit_reversed = false) {
    if (!handle_) return false;
    std::vector<const void*> data(leaves.size());
    std::vector<size_t> rows(leaves.size()), cols(leaves.size());
    for (size_t i = 0; i < leaves.size(); ++i) {
      data[i] = leaves[i].data;
      rows[i] = leaves[i].rows;
      cols[i] = leaves[i].cols;
    }
    const unsigned flags = bit_reversed ? TACHYON_MI355X_MERKLE_BIT_REVERSED : 0u;
    if (tachyon_mi355x_baby_bear_merkle_tree_build(handle_, data.data(), rows.data(), cols.data(), leaves.size(),
                                                   flags) != 1)
      return false;
    leaves_ = leaves;
    bit_reversed_ = bit_reversed;
    return true;
  }

  const std::vector<MatrixView<F>>& leaves() const { return leaves_; }
  bool bit_reversed() const { return bit_reversed_; }

  /* digest_layers().back()[0]; waits for the stream.  All zero before a build. */
  Digest GetRoot() const {
    Digest root{};
    if (handle_) (void)tachyon_mi355x_baby_bear_merkle_tree_root(handle_, root.data());
    return root;
  }

  /* a host copy of every layer, the leaf layer first */
  std::vector<std::vector<Digest>> digest_layers() const {
    std::vector<std::vector<Digest>> layers;
    const size_t n = handle_ ? tachyon_mi355x_baby_bear_merkle_tree_num_layers(handle_) : 0;
    for (size_t k = 0; k < n; ++k) {
      std::vector<Digest> layer(tachyon_mi355x_baby_bear_merkle_tree_layer_size(handle_, k));
      if (tachyon_mi355x_baby_bear_merkle_tree_layer(handle_, k, layer.data()) != 1) return {};
      layers.push_back(std::move(layer));
    }
    return layers;
  }

  /* FieldMerkleTreeMMCS::DoCreateOpeningProof: the opened row of every matrix
   * (the caller's order) and the siblings from the leaf layer up. */
  [[nodiscard]] bool CreateOpeningProof(size_t index, std::vector<std::vector<F>>* openings,
                                        std::vector<Digest>* proof) const {
    if (!handle_ || !openings || !proof) return false;
    const size_t n = tachyon_mi355x_baby_bear_merkle_tree_num_layers(handle_);
    if (n == 0) return false;
    std::vector<std::vector<F>> rows(leaves_.size());
    std::vector<void*> out(leaves_.size());
    for (size_t i = 0; i < leaves_.size(); ++i) {
      rows[i].resize(leaves_[i].cols);
      out[i] = rows[i].data();
    }
    std::vector<Digest> siblings(n - 1);
    Digest unused;
    if (tachyon_mi355x_baby_bear_merkle_tree_open(handle_, index, out.data(),
                                                  n > 1 ? siblings.data()->data() : unused.data()) != 1)
      return false;
    *openings = std::move(rows);
    *proof = std::move(siblings);
    return true;
  }

  const F* layers_device() const {
    return handle_ ? static_cast<const F*>(tachyon_mi355x_baby_bear_merkle_tree_layers_device_ptr(handle_)) : nullptr;
  }
  unsigned last_launches() const { return handle_ ? tachyon_mi355x_baby_bear_merkle_tree_last_launches(handle_) : 0; }
  void* stream() const { return handle_ ? tachyon_mi355x_baby_bear_merkle_tree_stream(handle_) : nullptr; }
  tachyon_mi355x_baby_bear_merkle_tree* handle() { return handle_; }

 private:
  tachyon_mi355x_baby_bear_merkle_tree* handle_ = nullptr;
  std::vector<MatrixView<F>> leaves_;
  bool bit_reversed_ = false;
};

/* TwoAdicFRI::Commit (two_adic_fri.h:76-94): the low-degree extension of every
 * matrix by log_blowup bits on the coset shift * <w>, then the commitment to
 * the extended matrices.  The reference extends with reverse_at_last = false
 * and commits the bit-reversed rows; here ldes[m] ((rows << log_blowup) x cols,
 * the caller's buffer) receives the natural-order extension and the tree is
 * built with bit-reversed leaves, which gives the same layers without a
 * permuted copy.  The tree is made on the holder's stream: with a holder
 * initialised for device buffers and is_async, nothing waits for the device
 * between the extension and the build, or before the call returns.  shift is
 * the field element as stored (Montgomery).  nullptr on refusal. */
template <class F>
std::unique_ptr<FieldMerkleTree<F>> Commit(const IcicleNTTHolder<F, kBabyBear>& holder,
                                           const std::vector<MatrixView<F>>& matrices, size_t log_blowup,
                                           const F& shift, const std::vector<F*>& ldes,
                                           Poseidon2ExternalMatrix external = Poseidon2ExternalMatrix::kHorizen) {
  if (!holder || !holder->stream() || matrices.empty() || ldes.size() != matrices.size()) return nullptr;
  auto tree = std::make_unique<FieldMerkleTree<F>>(external, holder->stream());
  std::vector<MatrixView<F>> extended(matrices.size());
  for (size_t m = 0; m < matrices.size(); ++m) {
    const MatrixView<F>& in = matrices[m];
    if (!in.data || !ldes[m] || !holder->CosetLDEBatch(in.data, in.rows, in.cols, log_blowup, shift, ldes[m]))
      return nullptr;
    extended[m] = MatrixView<F>{ldes[m], in.rows << log_blowup, in.cols};
  }
  if (!tree->Build(extended, /*bit_reversed=*/true)) return nullptr;
  return tree;
}

}  // namespace tachyon_mi355x

#endif  // TACHYON_MI355X_MERKLE_TREE_H_
