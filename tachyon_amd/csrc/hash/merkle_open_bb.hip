// FieldMerkleTreeMMCS's openings, at one index or many at once (see merkle_bb.h):
//   open_batch_kernel   block (q, job): job m < matrices copies the opened row
//                       of matrix m for query q, the lanes along its columns (a
//                       row is one contiguous run on both sides); the last job
//                       gathers the query's sibling digests, 8 lanes a digest
// The answer is gathered into one device buffer and leaves by one copy per
// output array.
#include <cstring>
#include <vector>

#include "merkle_bb.h"

namespace tachyon_amd::hash {

namespace {

constexpr unsigned kBlock = 256;
// the last job gathers a query's sibling digests with 8 lanes a digest in one block
static_assert((size_t(1) << (kBlock / 8)) >= merkle_tree::kMaxRows);

struct OpenMat {
  const uint32_t* src;
  uint64_t out_at;  // words before this matrix's rows in the answer
  uint32_t rows, cols;
  uint32_t log_rows;  // ceil_log2(rows)
  uint32_t pad;
};
static_assert(sizeof(OpenMat) == 32);

struct OpenArgs {
  const OpenMat* mats;
  const uint32_t* indices;
  const uint32_t* layers;
  uint32_t* out;
  uint64_t sib_at;  // words before the siblings in the answer
  uint32_t num_mats;
  uint32_t log_max;
  uint32_t bit_reversed;
};

__global__ __launch_bounds__(kBlock) void open_batch_kernel(const OpenArgs a) {
  const uint32_t q = blockIdx.x, job = blockIdx.y, t = threadIdx.x;
  const uint32_t index = a.indices[q];
  if (job < a.num_mats) {
    const OpenMat m = a.mats[job];
    // merkle_tree::open_row
    uint32_t r = index >> (a.log_max - m.log_rows);
    if (a.bit_reversed) r = m.log_rows ? __brev(r) >> (32 - m.log_rows) : 0u;
    const bool present = r < m.rows;
    const uint32_t* src = m.src + (size_t)r * m.cols;
    uint32_t* dst = a.out + m.out_at + (size_t)q * m.cols;
    for (uint32_t c = t; c < m.cols; c += kBlock) dst[c] = present ? src[c] : 0u;
    return;
  }
  gather_siblings(a.layers, a.log_max, index, a.out + a.sib_at + 8 * (size_t)q * a.log_max, t);
}

}  // namespace

bool BbMerkleTree::open(size_t index, void* const* rows_out, void* siblings_out) {
  return open_batch(&index, 1, rows_out, siblings_out);
}

bool BbMerkleTree::open_batch(const size_t* indices, size_t count, void* const* rows_out, void* siblings_out) {
  if (!built() || !indices || !rows_out || count == 0 || count > kMaxBatch) return false;
  if (plan_.log_max > 0 && !siblings_out) return false;
  const size_t num_mats = mats_.size();
  for (size_t m = 0; m < num_mats; ++m)
    if (!rows_out[m]) return false;
  for (size_t q = 0; q < count; ++q)
    if (indices[q] >= plan_.levels[0].size) return false;

  // what goes in: the indices, then the matrix records (16-byte aligned)
  const size_t idx_bytes = (count * sizeof(uint32_t) + 15) / 16 * 16;
  const size_t in_bytes = idx_bytes + num_mats * sizeof(OpenMat);
  std::vector<uint8_t> in(in_bytes);
  uint32_t* h_idx = reinterpret_cast<uint32_t*>(in.data());
  for (size_t q = 0; q < count; ++q) h_idx[q] = (uint32_t)indices[q];
  size_t words = 0;
  for (size_t m = 0; m < num_mats; ++m) {
    OpenMat rec{};
    rec.src = mats_[m];
    rec.out_at = words;
    rec.rows = (uint32_t)rows_[m];
    rec.cols = (uint32_t)cols_[m];
    rec.log_rows = merkle_tree::ceil_log2(rows_[m]);
    memcpy(in.data() + idx_bytes + m * sizeof(OpenMat), &rec, sizeof rec);
    words += count * cols_[m];
  }
  const size_t sib_at = words;
  words += count * plan_.log_max * kDigestWords;

  uint8_t* d = static_cast<uint8_t*>(batch_.ensure(in_bytes + words * sizeof(uint32_t)));
  TA_HIP(hipMemcpyAsync(d, in.data(), in_bytes, hipMemcpyHostToDevice, stream_));
  OpenArgs a{};
  a.mats = reinterpret_cast<const OpenMat*>(d + idx_bytes);
  a.indices = reinterpret_cast<const uint32_t*>(d);
  a.layers = layers_.as<uint32_t>();
  a.out = reinterpret_cast<uint32_t*>(d + in_bytes);
  a.sib_at = sib_at;
  a.num_mats = (uint32_t)num_mats;
  a.log_max = plan_.log_max;
  a.bit_reversed = (flags_ & merkle_tree::kFlagBitReversed) ? 1u : 0u;
  hipLaunchKernelGGL(open_batch_kernel, dim3((unsigned)count, (unsigned)num_mats + 1), dim3(kBlock), 0, stream_, a);
  TA_HIP(hipGetLastError());
  for (size_t m = 0, at = 0; m < num_mats; at += count * cols_[m], ++m)
    TA_HIP(hipMemcpyAsync(rows_out[m], a.out + at, count * cols_[m] * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          stream_));
  if (plan_.log_max > 0)
    TA_HIP(hipMemcpyAsync(siblings_out, a.out + sib_at, count * plan_.log_max * kDigestWords * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
  return true;
}

}  // namespace tachyon_amd::hash
