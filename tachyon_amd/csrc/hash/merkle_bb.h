// FieldMerkleTree<BabyBear, 8> on the GPU (field_merkle_tree.h,
// field_merkle_tree_mmcs.h): Poseidon2 width-16 PaddingFreeSponge<., 8, 8> leaf
// hashes, TruncatedPermutation<., 8, 2> compression, mixed heights, and the
// openings of FieldMerkleTreeMMCS.  Elements are Montgomery words
// (field/bb31.h); a digest is 8 consecutive words and the layers lie one after
// another in one device buffer, leaf layer first.
//
// build() only enqueues work on the tree's stream when every matrix is device
// memory: it can follow a CosetLDEBatch on the same stream without a host
// synchronisation.  Device matrices are referenced, not copied; the caller
// keeps them alive for open().  Host matrices are uploaded and kept.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../capi/merkle_tree_validate.h"
#include "../common/hip_util.h"

namespace tachyon_amd::hash {

// Poseidon2 on `count` states of 16 words, in place, device memory, enqueued on
// `stream`.  external: 0 Horizen, 1 Plonky3.
void poseidon2_bb_permute(int external, uint32_t* d_states, size_t count, hipStream_t stream);

// in-register bb31::mul rate (products per second) of `iters` dependent
// products in each of `threads` lanes: the VALU yardstick of the probe
double bb31_mul_rate(size_t threads, unsigned iters, hipStream_t stream);

// The sibling digests on the path from leaf `index` of a tree of 2^log_leaves
// leaves whose layers lie in `layers` as BbMerkleTree keeps them (layer k
// begins 2 leaves - (2 leaves >> k) digests in): the sibling in layer k goes to
// dst + 8 k, 8 lanes a digest, so lane t writes word t.  Every lane of a block
// of at least 8 log_leaves lanes calls it with its own `lane`.
__device__ __forceinline__ void gather_siblings(const uint32_t* layers, uint32_t log_leaves, uint32_t index,
                                                uint32_t* dst, uint32_t lane) {
  if (lane < 8 * log_leaves) {
    const uint32_t k = lane / 8, j = lane % 8;
    const size_t leaves = size_t(1) << log_leaves;
    const size_t offset = 2 * leaves - ((2 * leaves) >> k);  // digests before layer k
    const size_t sibling = (index >> k) ^ 1;
    dst[lane] = layers[8 * (offset + sibling) + j];
  }
}

class BbMerkleTree {
 public:
  static constexpr size_t kDigestWords = 8;
  static constexpr size_t kTailSize = 256;  // layers up to this size are finished by one workgroup

  BbMerkleTree(int external, hipStream_t stream);
  ~BbMerkleTree();
  BbMerkleTree(const BbMerkleTree&) = delete;
  BbMerkleTree& operator=(const BbMerkleTree&) = delete;

  // False (and the tree keeps what it held) when merkle_tree::make_plan refuses
  // the shapes or a pointer is null.  Throws on a HIP error; when the layer
  // buffer cannot be allocated the tree is left without a build.
  bool build(const void* const* mats, const size_t* rows, const size_t* cols, size_t count, unsigned flags);

  bool built() const { return !plan_.levels.empty(); }
  size_t num_layers() const { return plan_.levels.size(); }
  size_t layer_size(size_t k) const { return k < plan_.levels.size() ? plan_.levels[k].size : 0; }
  size_t num_matrices() const { return rows_.size(); }
  const uint32_t* layers_device() const { return built() ? layers_.as<uint32_t>() : nullptr; }
  hipStream_t stream() const { return stream_; }
  unsigned last_launches() const { return launches_; }

  // copies to host memory; they wait for the stream
  bool layer(size_t k, void* out);
  bool root(void* out);
  // rows_out[m]: cols[m] words of matrix m (the caller's order), zeros for a row
  // past its height; siblings_out: (num_layers - 1) digests.  False for
  // index >= layer_size(0).  It is open_batch at one index.
  bool open(size_t index, void* const* rows_out, void* siblings_out);
  // open() at `count` indices (merkle_open_bb.hip): rows_out[m] receives count
  // rows of cols[m] words, siblings_out count * (num_layers - 1) digests, query
  // q's part what open(indices[q]) writes.  One gather launch, one copy per
  // output array, one wait.  False, with nothing written, for a null pointer,
  // count 0 or above kMaxBatch, or an index >= layer_size(0).
  static constexpr size_t kMaxBatch = size_t(1) << 16;
  bool open_batch(const size_t* indices, size_t count, void* const* rows_out, void* siblings_out);

  // the last build's arguments, the caller's order (device pointers)
  int external() const { return external_; }
  unsigned flags() const { return flags_; }
  unsigned log_max() const { return plan_.log_max; }
  const void* matrix(size_t m) const { return m < mats_.size() ? mats_[m] : nullptr; }
  size_t matrix_rows(size_t m) const { return m < rows_.size() ? rows_[m] : 0; }
  size_t matrix_cols(size_t m) const { return m < cols_.size() ? cols_[m] : 0; }

 private:
  int external_;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  merkle_tree::Plan plan_;
  unsigned flags_ = 0;
  std::vector<const uint32_t*> mats_;  // device pointers, the caller's order
  std::vector<size_t> rows_, cols_;
  std::vector<std::unique_ptr<DeviceBuffer>> uploads_;  // host matrices' device copies
  DeviceBuffer layers_;                // the layers, then the injected hashes of levels >= 1
  unsigned launches_ = 0;
  DeviceBuffer batch_;                 // open_batch: indices and matrix records in, the gathered answer out
};

}  // namespace tachyon_amd::hash
