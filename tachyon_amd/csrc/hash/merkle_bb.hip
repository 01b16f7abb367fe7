// Poseidon2 / FieldMerkleTree kernels for BabyBear (see merkle_bb.h,
// poseidon2_bb.h).  Three kernels and a tail:
//   permute_kernel   a batch of states in place, one state per lane
//   hash_kernel      PaddingFreeSponge of the concatenated rows of up to
//                    kMaxGroup equal-height matrices.  A workgroup stages a
//                    tile of kTileRows rows x kTileCols concatenated columns
//                    through LDS with coalesced loads (lanes along the
//                    columns), pitch kTileCols + 1 so that lanes reading their
//                    own row hit distinct banks; each lane then absorbs its
//                    row 8 words at a time.
//   layer_kernel     next[i] = C(prev[2i], prev[2i+1]), or with an injected
//                    layer C(C(prev[2i], prev[2i+1]), i < rows ? H_i : 0)
//   tail_kernel      every layer of at most kTailSize digests, by one
//                    workgroup, instead of one launch of a few lanes per layer
#include "merkle_bb.h"

#include <memory>
#include <type_traits>

#include "poseidon2_bb.h"

namespace tachyon_amd::hash {

namespace p2 = poseidon2_bb;

namespace {

constexpr unsigned kBlock = 256;
constexpr unsigned kTileRows = kBlock;
constexpr unsigned kTileCols = 32;  // 4 absorptions per staged tile
constexpr unsigned kPitch = kTileCols + 1;
constexpr unsigned kMaxTailLevels = 9;  // prev layer <= 2 * kTailSize = 2^9 digests
static_assert(BbMerkleTree::kTailSize == kBlock && (size_t(2) * BbMerkleTree::kTailSize) >> kMaxTailLevels == 1);

struct HashArgs {
  const uint32_t* mat[merkle_tree::kMaxGroup];
  uint32_t cols[merkle_tree::kMaxGroup];
  uint32_t col_begin[merkle_tree::kMaxGroup + 1];  // concatenated column where matrix m starts
  uint32_t count;
  uint32_t total_cols;
  uint32_t rows;       // rows hashed
  uint32_t out_count;  // digests written: zeros for rows <= i < out_count
  uint32_t log_rows;   // bit-reversed leaves: leaf i is the stored row bitrev(i) over log_rows bits
  uint32_t bit_reversed;
  uint32_t* out;
};

struct TailArgs {
  uint32_t* prev;   // the last layer already built; the next ones follow it
  uint32_t n_prev;  // its size, a power of two <= 2 * kTailSize
  const uint32_t* inject[kMaxTailLevels];  // per next layer: hashes to inject or null
  uint32_t inject_rows[kMaxTailLevels];
};

__device__ __forceinline__ void store_digest(uint32_t* out, const uint32_t* s) {
  uint4* o = reinterpret_cast<uint4*>(out);
  o[0] = make_uint4(s[0], s[1], s[2], s[3]);
  o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

__device__ __forceinline__ void load_digest(const uint32_t* in, uint32_t* s) {
  const uint4* p = reinterpret_cast<const uint4*>(in);
  const uint4 a = p[0], b = p[1];
  s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
  s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
}

template <int EXT>
__global__ __launch_bounds__(kBlock) void permute_kernel(uint32_t* states, size_t count) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  uint32_t s[16];
  uint32_t* x = states + 16 * i;
#pragma unroll
  for (int j = 0; j < 16; ++j) s[j] = x[j];
  p2::permute<EXT>(s);
#pragma unroll
  for (int j = 0; j < 16; ++j) x[j] = s[j];
}

template <int EXT>
__global__ __launch_bounds__(kBlock) void hash_kernel(const HashArgs a) {
  __shared__ uint32_t tile[kTileRows * kPitch];
  const uint32_t t = threadIdx.x;
  const uint32_t row0 = blockIdx.x * kTileRows;
  const uint32_t my_row = row0 + t;
  // this lane's column of the tile is the same in every step of the staging loop
  const uint32_t lc = t % kTileCols;
  const uint32_t lr0 = t / kTileCols;
  constexpr uint32_t kRowStep = kBlock / kTileCols;

  uint32_t s[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) s[j] = 0;

#pragma unroll 1
  for (uint32_t c0 = 0; c0 < a.total_cols; c0 += kTileCols) {
    const uint32_t c = c0 + lc;
    // the matrix and the column in it that concatenated column c belongs to
    const uint32_t* src = nullptr;
    uint32_t mcols = 0, mcol = 0;
    if (c < a.total_cols) {
      uint32_t m = 0;
      while (m + 1 < a.count && c >= a.col_begin[m + 1]) ++m;
      src = a.mat[m];
      mcols = a.cols[m];
      mcol = c - a.col_begin[m];
    }
    __syncthreads();  // the previous tile has been absorbed
    if (src) {
#pragma unroll 4
      for (uint32_t lr = lr0; lr < kTileRows; lr += kRowStep) {
        const uint32_t r = row0 + lr;
        if (r < a.rows) {
          const uint32_t stored = a.bit_reversed ? (a.log_rows ? __brev(r) >> (32 - a.log_rows) : 0u) : r;
          tile[lr * kPitch + lc] = src[(size_t)stored * mcols + mcol];
        }
      }
    }
    __syncthreads();
    if (my_row < a.rows) {
      const uint32_t* mine = tile + t * kPitch;
#pragma unroll 1
      for (uint32_t at = 0; at < kTileCols && c0 + at < a.total_cols; at += 8) {
        const uint32_t k = a.total_cols - (c0 + at);  // words present, >= 1; a short chunk keeps the other lanes
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
          if (j < k) s[j] = mine[at + j];
        p2::permute<EXT>(s);
      }
    }
  }
  if (my_row < a.out_count) {
    if (my_row >= a.rows) {
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] = 0;
    }
    store_digest(a.out + 8 * (size_t)my_row, s);
  }
}

// next[i] from prev[2i], prev[2i + 1] and, with `inject`, the hash of row i
template <int EXT>
__device__ __forceinline__ void compress_item(const uint32_t* prev, const uint32_t* inject, uint32_t inject_rows,
                                               uint32_t i, uint32_t* next) {
  uint32_t s[16];
  load_digest(prev + 16 * (size_t)i, s);
  load_digest(prev + 16 * (size_t)i + 8, s + 8);
  const int passes = inject ? 2 : 1;
#pragma unroll 1
  for (int pass = 0; pass < passes; ++pass) {
    if (pass) {
      if (i < inject_rows) {
        load_digest(inject + 8 * (size_t)i, s + 8);
      } else {
#pragma unroll
        for (int j = 8; j < 16; ++j) s[j] = 0;
      }
    }
    p2::permute<EXT>(s);
  }
  store_digest(next + 8 * (size_t)i, s);
}

template <int EXT>
__global__ __launch_bounds__(kBlock) void layer_kernel(const uint32_t* prev, const uint32_t* inject,
                                                       uint32_t inject_rows, uint32_t n_next, uint32_t* next) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n_next) compress_item<EXT>(prev, inject, inject_rows, i, next);
}

template <int EXT>
__global__ __launch_bounds__(kBlock) void tail_kernel(const TailArgs a) {
  uint32_t* prev = a.prev;
  uint32_t level = 0;
#pragma unroll 1
  for (uint32_t n = a.n_prev / 2; n >= 1; n /= 2, ++level) {
    uint32_t* next = prev + 8 * (size_t)(2 * n);
    if (threadIdx.x < n) compress_item<EXT>(prev, a.inject[level], a.inject_rows[level], threadIdx.x, next);
    __syncthreads();  // the layer is visible to the workgroup before it is read
    prev = next;
  }
}

__global__ __launch_bounds__(kBlock) void mul_rate_kernel(uint32_t* out, uint32_t iters) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  // four independent chains per lane, as the s-box offers across lanes of the state
  uint32_t a = i % bb31::kP, b = (i + 1) % bb31::kP, c = (i + 2) % bb31::kP, d = (i + 3) % bb31::kP;
#pragma unroll 4
  for (uint32_t k = 0; k < iters; ++k) {
    a = bb31::mul(a, b);
    b = bb31::mul(b, c);
    c = bb31::mul(c, d);
    d = bb31::mul(d, a);
  }
  out[i] = a ^ b ^ c ^ d;
}

template <class Fn>
void with_external(int external, Fn&& fn) {
  if (external == p2::kHorizen) fn(std::integral_constant<int, p2::kHorizen>{});
  else fn(std::integral_constant<int, p2::kPlonky3>{});
}

}  // namespace

void poseidon2_bb_permute(int external, uint32_t* d_states, size_t count, hipStream_t stream) {
  if (count == 0) return;
  with_external(external, [&](auto ext) {
    hipLaunchKernelGGL(permute_kernel<decltype(ext)::value>, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, stream,
                       d_states, count);
  });
  TA_HIP(hipGetLastError());
}

double bb31_mul_rate(size_t threads, unsigned iters, hipStream_t stream) {
  const unsigned blocks = ceil_div(threads, kBlock);
  DeviceBuffer out;
  out.ensure((size_t)blocks * kBlock * sizeof(uint32_t));
  hipEvent_t e0, e1;
  TA_HIP(hipEventCreate(&e0));
  TA_HIP(hipEventCreate(&e1));
  float best = 0;
  for (int rep = 0; rep < 4; ++rep) {  // the first run warms up
    TA_HIP(hipEventRecord(e0, stream));
    hipLaunchKernelGGL(mul_rate_kernel, dim3(blocks), dim3(kBlock), 0, stream, out.as<uint32_t>(), iters);
    TA_HIP(hipEventRecord(e1, stream));
    TA_HIP(hipEventSynchronize(e1));
    float ms = 0;
    TA_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (rep && (best == 0 || ms < best)) best = ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return 4.0 * iters * blocks * kBlock / (best * 1e-3);
}

BbMerkleTree::BbMerkleTree(int external, hipStream_t stream) : external_(external), stream_(stream) {
  require_gpu();
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
}

BbMerkleTree::~BbMerkleTree() {
  (void)hipStreamSynchronize(stream_);
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

bool BbMerkleTree::build(const void* const* mats, const size_t* rows, const size_t* cols, size_t count,
                         unsigned flags) {
  merkle_tree::Plan plan;
  if (!mats || !merkle_tree::make_plan(rows, cols, count, flags, &plan)) return false;
  for (size_t i = 0; i < count; ++i)
    if (!mats[i]) return false;

  // host matrices are uploaded; device matrices are used where they are
  std::vector<const uint32_t*> dev(count);
  std::vector<std::unique_ptr<DeviceBuffer>> uploads;
  bool uploaded = false;
  for (size_t i = 0; i < count; ++i) {
    if (is_device_pointer(mats[i])) {
      dev[i] = static_cast<const uint32_t*>(mats[i]);
      continue;
    }
    const size_t bytes = rows[i] * cols[i] * sizeof(uint32_t);
    uploads.push_back(std::make_unique<DeviceBuffer>());
    void* d = uploads.back()->ensure(bytes);
    TA_HIP(hipMemcpyAsync(d, mats[i], bytes, hipMemcpyHostToDevice, stream_));
    dev[i] = static_cast<const uint32_t*>(d);
    uploaded = true;
  }
  if (uploaded) TA_HIP(hipStreamSynchronize(stream_));  // the host buffers are the caller's again

  // layers (2 size_0 - 1 digests), then room for the injected hashes of the
  // levels >= 1 at the same offsets less size_0
  const size_t size0 = plan.levels[0].size;
  const size_t total = 2 * size0 - 1;
  // (growing the buffer frees the old one, which waits for the device)
  uint32_t* layers;
  try {
    layers = static_cast<uint32_t*>(layers_.ensure((total + size0) * kDigestWords * sizeof(uint32_t)));
  } catch (...) {
    plan_ = merkle_tree::Plan();  // the old buffer is gone: no tree rather than one without layers
    throw;
  }
  uint32_t* inject_base = layers + total * kDigestWords;

  plan_ = std::move(plan);
  flags_ = flags;
  mats_ = std::move(dev);
  rows_.assign(rows, rows + count);
  cols_.assign(cols, cols + count);
  uploads_ = std::move(uploads);
  launches_ = 0;

  auto hash_level = [&](const merkle_tree::Level& l, uint32_t* out, size_t out_count) {
    HashArgs a{};
    uint32_t at = 0;
    for (size_t m = 0; m < l.count; ++m) {
      const size_t id = plan_.order[l.first + m];
      a.mat[m] = mats_[id];
      a.cols[m] = (uint32_t)cols_[id];
      a.col_begin[m] = at;
      at += (uint32_t)cols_[id];
    }
    a.col_begin[l.count] = at;
    a.count = (uint32_t)l.count;
    a.total_cols = at;
    a.rows = (uint32_t)l.rows;
    a.out_count = (uint32_t)out_count;
    a.log_rows = merkle_tree::ceil_log2(l.rows);
    a.bit_reversed = (flags_ & merkle_tree::kFlagBitReversed) ? 1u : 0u;
    a.out = out;
    with_external(external_, [&](auto ext) {
      hipLaunchKernelGGL(hash_kernel<decltype(ext)::value>, dim3(ceil_div(out_count, kTileRows)), dim3(kBlock), 0,
                         stream_, a);
    });
    ++launches_;
  };

  // every hash first: the leaf layer, then the layers to inject
  hash_level(plan_.levels[0], layers, size0);
  std::vector<const uint32_t*> inject(plan_.levels.size(), nullptr);
  for (size_t k = 1; k < plan_.levels.size(); ++k) {
    const merkle_tree::Level& l = plan_.levels[k];
    if (!l.count) continue;
    uint32_t* out = inject_base + (merkle_tree::layer_offset(plan_, k) - size0) * kDigestWords;
    hash_level(l, out, l.rows);
    inject[k] = out;
  }

  uint32_t* prev = layers;
  for (size_t k = 1; k < plan_.levels.size(); ++k) {
    const merkle_tree::Level& l = plan_.levels[k];
    if (l.size <= kTailSize) {
      TailArgs t{};
      t.prev = prev;
      t.n_prev = (uint32_t)(2 * l.size);
      for (size_t j = k; j < plan_.levels.size(); ++j) {
        t.inject[j - k] = inject[j];
        t.inject_rows[j - k] = (uint32_t)plan_.levels[j].rows;
      }
      with_external(external_, [&](auto ext) {
        hipLaunchKernelGGL(tail_kernel<decltype(ext)::value>, dim3(1), dim3(kBlock), 0, stream_, t);
      });
      ++launches_;
      break;
    }
    uint32_t* next = prev + 2 * l.size * kDigestWords;
    with_external(external_, [&](auto ext) {
      hipLaunchKernelGGL(layer_kernel<decltype(ext)::value>, dim3(ceil_div(l.size, kBlock)), dim3(kBlock), 0, stream_,
                         prev, inject[k], (uint32_t)l.rows, (uint32_t)l.size, next);
    });
    ++launches_;
    prev = next;
  }
  TA_HIP(hipGetLastError());
  return true;
}

bool BbMerkleTree::layer(size_t k, void* out) {
  if (!built() || k >= plan_.levels.size() || !out) return false;
  const uint32_t* src = layers_.as<uint32_t>() + merkle_tree::layer_offset(plan_, k) * kDigestWords;
  TA_HIP(hipMemcpyAsync(out, src, plan_.levels[k].size * kDigestWords * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        stream_));
  TA_HIP(hipStreamSynchronize(stream_));
  return true;
}

bool BbMerkleTree::root(void* out) { return built() && layer(plan_.levels.size() - 1, out); }

}  // namespace tachyon_amd::hash
