// C-ABI of Poseidon2 over BabyBear and FieldMerkleTree<BabyBear, 8>
// (include/tachyon_mi355x.h) over hash::BbMerkleTree: int results, nothing
// aborts across this boundary.  The shape rules live in merkle_tree_validate.h.
#include "../../../include/tachyon_mi355x.h"

#include <memory>

#include "../common/hip_util.h"
#include "../hash/merkle_bb.h"
#include "capi_handles.h"
#include "merkle_tree_validate.h"

using namespace tachyon_amd;

static_assert(TACHYON_MI355X_MERKLE_BIT_REVERSED == merkle_tree::kFlagBitReversed);

extern "C" {

int tachyon_mi355x_poseidon2_baby_bear_permute(int external_matrix, void* states, size_t count, void* stream) {
  if (!merkle_tree::external_ok(external_matrix) || !states || count == 0 || count > (size_t(1) << 32)) return 0;
  return guarded(0, [&] {
    require_gpu();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (is_device_pointer(states)) {
      hash::poseidon2_bb_permute(external_matrix, static_cast<uint32_t*>(states), count, s);
      if (!s) TA_HIP(hipStreamSynchronize(s));
      return 1;
    }
    const size_t bytes = count * 16 * sizeof(uint32_t);
    DeviceBuffer d;
    d.ensure(bytes);
    TA_HIP(hipMemcpyAsync(d.as<void>(), states, bytes, hipMemcpyHostToDevice, s));
    hash::poseidon2_bb_permute(external_matrix, d.as<uint32_t>(), count, s);
    TA_HIP(hipMemcpyAsync(states, d.as<void>(), bytes, hipMemcpyDeviceToHost, s));
    TA_HIP(hipStreamSynchronize(s));
    return 1;
  });
}

tachyon_mi355x_baby_bear_merkle_tree* tachyon_mi355x_baby_bear_merkle_tree_create(int external_matrix, void* stream) {
  if (!merkle_tree::external_ok(external_matrix)) return nullptr;
  return guarded<tachyon_mi355x_baby_bear_merkle_tree*>(nullptr, [&] {
    auto h = std::make_unique<tachyon_mi355x_baby_bear_merkle_tree>();
    h->tree = std::make_unique<hash::BbMerkleTree>(external_matrix, static_cast<hipStream_t>(stream));
    return h.release();
  });
}

void tachyon_mi355x_baby_bear_merkle_tree_destroy(tachyon_mi355x_baby_bear_merkle_tree* tree) {
  try {
    delete tree;
  } catch (...) {
  }
}

int tachyon_mi355x_baby_bear_merkle_tree_build(tachyon_mi355x_baby_bear_merkle_tree* tree,
                                               const void* const* matrices, const size_t* rows, const size_t* cols,
                                               size_t count, unsigned flags) {
  if (!tree || !matrices || !rows || !cols || count == 0) return 0;
  return guarded(0, [&] { return tree->tree->build(matrices, rows, cols, count, flags); });
}

int tachyon_mi355x_baby_bear_merkle_tree_root(tachyon_mi355x_baby_bear_merkle_tree* tree, void* out) {
  if (!tree || !out) return 0;
  return guarded(0, [&] { return tree->tree->root(out); });
}

size_t tachyon_mi355x_baby_bear_merkle_tree_num_layers(const tachyon_mi355x_baby_bear_merkle_tree* tree) {
  return tree ? tree->tree->num_layers() : 0;
}

size_t tachyon_mi355x_baby_bear_merkle_tree_layer_size(const tachyon_mi355x_baby_bear_merkle_tree* tree, size_t k) {
  return tree ? tree->tree->layer_size(k) : 0;
}

int tachyon_mi355x_baby_bear_merkle_tree_layer(tachyon_mi355x_baby_bear_merkle_tree* tree, size_t k, void* out) {
  if (!tree || !out) return 0;
  return guarded(0, [&] { return tree->tree->layer(k, out); });
}

const void* tachyon_mi355x_baby_bear_merkle_tree_layers_device_ptr(const tachyon_mi355x_baby_bear_merkle_tree* tree) {
  return tree ? tree->tree->layers_device() : nullptr;
}

int tachyon_mi355x_baby_bear_merkle_tree_open(tachyon_mi355x_baby_bear_merkle_tree* tree, size_t index,
                                              void* const* rows_out, void* siblings_out) {
  if (!tree || !rows_out) return 0;
  return guarded(0, [&] { return tree->tree->open(index, rows_out, siblings_out); });
}

unsigned tachyon_mi355x_baby_bear_merkle_tree_last_launches(const tachyon_mi355x_baby_bear_merkle_tree* tree) {
  return tree ? tree->tree->last_launches() : 0;
}

void* tachyon_mi355x_baby_bear_merkle_tree_stream(tachyon_mi355x_baby_bear_merkle_tree* tree) {
  return tree ? static_cast<void*>(tree->tree->stream()) : nullptr;
}

double tachyon_mi355x_baby_bear_mul_rate(size_t threads, unsigned iters) {
  if (threads == 0 || iters == 0 || threads > (size_t(1) << 28)) return 0;
  return guarded(0.0, [&] {
    require_gpu();
    return hash::bb31_mul_rate(threads, iters, nullptr);
  });
}

}  // extern "C"
