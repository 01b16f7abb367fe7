// The FRI opening's kernels for BabyBear / BabyBear4 (see fri_bb.h):
//   ops_kernel          elementwise BabyBear4 arithmetic (the field's device test)
//   alpha_pow_kernel    alpha^c for the columns of the widest matrix so far
//   inv_denoms_kernel   (x_i - z)^-1 over 31 <w_n> in bit-reversed order; a zero
//                       difference sets the flag
//   interp_kernel       partial sums of sum_r (z_p - x_r)^-1 w_m^r M[r << lb][c]
//                       for up to kPointGroup points: 64 lanes along the
//                       columns (coalesced), 4 row lanes, the per-row
//                       coefficients of a 64-row tile in LDS, the sums in
//                       registers
//   finish_kernel       ys[p][c] = scale_p * the partial sums
//   reduced_ys_kernel   per point: sum_c alpha^c ys[c]
//   reduce_kernel       rr[i] = sum_c alpha^c M[bitrev(i)][c], a lane per
//                       position over tiles of 256 x 32 words staged through
//                       LDS as merkle_bb.hip's hash_kernel does, then
//                       ro[i] += sum_p alpha^offset_p (rr[i] - rys_p) inv_p[i]
//   fold_kernel         FoldMatrix plus the equal-size input
#include "fri_bb.h"

#include <cstring>

namespace tachyon_amd::fri {

namespace f4 = bb31x4;

namespace {

constexpr unsigned kBlock = 256;
constexpr unsigned kInterpCols = 64;   // columns of an interpolation block (lanes along them)
constexpr unsigned kInterpTile = 64;   // rows whose coefficients are staged at a time
constexpr unsigned kInterpBlocks = 2048;  // at most about this many interpolation blocks per launch
constexpr unsigned kTileRows = kBlock;  // positions of a reduce block, one lane each
constexpr unsigned kTileCols = 32;     // columns staged at a time
constexpr unsigned kPitch = kTileCols + 1;

// base^(2^j), Montgomery: the power of any exponent is a product over its set bits
struct PowTable {
  uint32_t w[kMaxLogRows + 1];
};

// one opening point of one matrix; apo, scale and inv come from the host, rys
// from reduced_ys_kernel
struct PointDev {
  Fp4 apo;    // alpha^offset
  Fp4 rys;    // sum_c alpha^c ys[c]
  Fp4 scale;  // (z^m - g^m) / (m g^(m-1))
  const Fp4* inv;  // (x_i - z)^-1, bit-reversed order
  uint64_t pad;
};
static_assert(sizeof(PointDev) == 64);

__device__ __forceinline__ uint32_t pow_bits(const PowTable& t, uint32_t e, uint32_t bits) {
  uint32_t r = bb31::kR;
  for (uint32_t j = 0; j < bits; ++j)
    if ((e >> j) & 1) r = bb31::mul(r, t.w[j]);
  return r;
}

// i reversed over `bits` bits (0 for bits == 0)
__device__ __forceinline__ uint32_t bitrev(uint32_t i, uint32_t bits) { return bits ? __brev(i) >> (32 - bits) : 0u; }

__device__ __forceinline__ Fp4 load4(const Fp4* p) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  return Fp4{{v.x, v.y, v.z, v.w}};
}

__device__ __forceinline__ void store4(Fp4* p, const Fp4& a) {
  *reinterpret_cast<uint4*>(p) = make_uint4(a.c[0], a.c[1], a.c[2], a.c[3]);
}

__global__ __launch_bounds__(kBlock) void ops_kernel(int op, const Fp4* a, const Fp4* b, Fp4* out, size_t count) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const Fp4 x = load4(a + i);
  Fp4 r;
  switch (op) {
    case kBb4Add: r = f4::add(x, load4(b + i)); break;
    case kBb4Sub: r = f4::sub(x, load4(b + i)); break;
    case kBb4Mul: r = f4::mul(x, load4(b + i)); break;
    case kBb4Square: r = f4::square(x); break;
    default: r = f4::inverse(x); break;
  }
  store4(out + i, r);
}

__global__ __launch_bounds__(kBlock) void alpha_pow_kernel(const Fp4 alpha, uint32_t count, Fp4* out) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c < count) store4(out + c, f4::pow(alpha, c));
}

__global__ __launch_bounds__(kBlock) void inv_denoms_kernel(const Fp4 z, const PowTable wn, uint32_t g, uint32_t log_n,
                                                            Fp4* out, uint32_t* flag) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= (1u << log_n)) return;
  const uint32_t x = bb31::mul(g, pow_bits(wn, bitrev(i, log_n), log_n));
  const Fp4 d = f4::sub(f4::from_base(x), z);
  if (f4::is_zero(d)) *flag = 1u;
  store4(out + i, f4::inverse(d));
}

struct InterpArgs {
  const uint32_t* mat;
  uint32_t cols, log_m, log_blowup;
  uint32_t rows_per_block;  // a multiple of kInterpTile, or all m rows
  uint32_t num_points;      // 1 .. PG
  const PointDev* pts;
  PowTable wm;
  Fp4* partial;  // [row block][point][col]
};

template <int PG>
__global__ __launch_bounds__(kBlock) void interp_kernel(const InterpArgs a) {
  __shared__ Fp4 coef[PG][kInterpTile];
  __shared__ Fp4 red[3][PG][kInterpCols];
  const uint32_t t = threadIdx.x, tx = t % kInterpCols, ty = t / kInterpCols;
  const uint32_t c = blockIdx.y * kInterpCols + tx;
  const uint32_t m = 1u << a.log_m;
  const uint32_t r_begin = blockIdx.x * a.rows_per_block;
  const uint32_t r_end = min(m, r_begin + a.rows_per_block);
  Fp4 acc[PG];
#pragma unroll
  for (int p = 0; p < PG; ++p) acc[p] = f4::zero();

#pragma unroll 1
  for (uint32_t r0 = r_begin; r0 < r_end; r0 += kInterpTile) {
    __syncthreads();  // the previous tile's coefficients have been used
    for (uint32_t item = t; item < PG * kInterpTile; item += kBlock) {
      const uint32_t p = item / kInterpTile, rl = item % kInterpTile, r = r0 + rl;
      if (p < a.num_points && r < r_end) {
        // (z - x_r)^-1 w_m^r: x_r = g w_m^r sits at position bitrev(r, log m) of the prefix
        const Fp4 d = load4(a.pts[p].inv + bitrev(r, a.log_m));
        coef[p][rl] = f4::neg(f4::mul_base(d, pow_bits(a.wm, r, a.log_m)));
      }
    }
    __syncthreads();
    if (c < a.cols) {
#pragma unroll 2
      for (uint32_t rl = ty; rl < kInterpTile && r0 + rl < r_end; rl += kBlock / kInterpCols) {
        const uint32_t v = a.mat[((size_t)(r0 + rl) << a.log_blowup) * a.cols + c];
#pragma unroll
        for (int p = 0; p < PG; ++p)
          if (p < (int)a.num_points) acc[p] = f4::add(acc[p], f4::mul_base(coef[p][rl], v));
      }
    }
  }
  // the four row lanes of a column into one
  if (ty > 0) {
#pragma unroll
    for (int p = 0; p < PG; ++p) red[ty - 1][p][tx] = acc[p];
  }
  __syncthreads();
  if (ty == 0 && c < a.cols) {
#pragma unroll
    for (int p = 0; p < PG; ++p) {
      if (p < (int)a.num_points) {
        Fp4 s = acc[p];
        for (int k = 0; k < 3; ++k) s = f4::add(s, red[k][p][tx]);
        store4(a.partial + ((size_t)blockIdx.x * a.num_points + p) * a.cols + c, s);
      }
    }
  }
}

// ys[p][c] = scale_p * the sum of the row blocks' partial sums: 16 lanes along
// the columns, 16 lanes over the row blocks of a column
__global__ __launch_bounds__(kBlock) void finish_kernel(const Fp4* partial, uint32_t row_blocks, uint32_t num_points,
                                                        uint32_t cols, const PointDev* pts, Fp4* ys) {
  constexpr uint32_t kLanes = 16;
  __shared__ Fp4 red[kLanes][kLanes];
  const uint32_t p = blockIdx.y, tx = threadIdx.x % kLanes, ty = threadIdx.x / kLanes;
  const uint32_t c = blockIdx.x * kLanes + tx;
  Fp4 s = f4::zero();
  if (c < cols) {
#pragma unroll 4
    for (uint32_t b = ty; b < row_blocks; b += kLanes)
      s = f4::add(s, load4(partial + ((size_t)b * num_points + p) * cols + c));
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < cols) {
    for (uint32_t k = 1; k < kLanes; ++k) s = f4::add(s, red[k][tx]);
    store4(ys + (size_t)p * cols + c, f4::mul(s, load4(&pts[p].scale)));
  }
}

// one block per point: rys = sum_c alpha^c ys[c]
__global__ __launch_bounds__(kBlock) void reduced_ys_kernel(const Fp4* ys, uint32_t cols, const Fp4* apow,
                                                            PointDev* pts) {
  __shared__ Fp4 red[kBlock];
  const uint32_t p = blockIdx.x, t = threadIdx.x;
  Fp4 acc = f4::zero();
  for (uint32_t c = t; c < cols; c += kBlock)
    acc = f4::add(acc, f4::mul(load4(apow + c), load4(ys + (size_t)p * cols + c)));
  red[t] = acc;
  __syncthreads();
  for (uint32_t s = kBlock / 2; s > 0; s /= 2) {
    if (t < s) red[t] = f4::add(red[t], red[t + s]);
    __syncthreads();
  }
  if (t == 0) store4(&pts[p].rys, red[0]);
}

struct ReduceArgs {
  const uint32_t* mat;
  uint32_t cols, log_n;
  uint32_t num_points;
  const Fp4* apow;
  const PointDev* pts;
  Fp4* ro;
};

// A workgroup stages a tile of kTileRows positions x kTileCols columns through
// LDS with coalesced loads (lanes along the columns of the natural row
// bitrev(i)), pitch kTileCols + 1 so that lanes reading their own row hit
// distinct banks; each lane then adds its row's part of sum_c alpha^c M[.][c],
// every lane reading the same alpha power from LDS (a broadcast).
__global__ __launch_bounds__(kBlock) void reduce_kernel(const ReduceArgs a) {
  __shared__ uint32_t tile[kTileRows * kPitch];
  __shared__ Fp4 apow[kTileCols];
  const uint32_t t = threadIdx.x;
  const uint32_t n = 1u << a.log_n;
  const uint32_t row0 = blockIdx.x * kTileRows;
  const uint32_t mine = row0 + t;
  const uint32_t lc = t % kTileCols, lr0 = t / kTileCols;
  constexpr uint32_t kRowStep = kBlock / kTileCols;
  Fp4 rr = f4::zero();

#pragma unroll 1
  for (uint32_t c0 = 0; c0 < a.cols; c0 += kTileCols) {
    const uint32_t c = c0 + lc;
    __syncthreads();  // the previous tile has been used
    if (t < kTileCols && c0 + t < a.cols) apow[t] = load4(a.apow + c0 + t);
    if (c < a.cols) {
#pragma unroll 4
      for (uint32_t lr = lr0; lr < kTileRows; lr += kRowStep) {
        const uint32_t i = row0 + lr;
        if (i < n) tile[lr * kPitch + lc] = a.mat[(size_t)bitrev(i, a.log_n) * a.cols + c];
      }
    }
    __syncthreads();
    if (mine < n) {
      const uint32_t* my = tile + t * kPitch;
      const uint32_t k = min(kTileCols, a.cols - c0);
#pragma unroll 4
      for (uint32_t j = 0; j < k; ++j) rr = f4::add(rr, f4::mul_base(apow[j], my[j]));
    }
  }
  if (mine < n) {
    Fp4 ro = load4(a.ro + mine);
    for (uint32_t p = 0; p < a.num_points; ++p) {
      const PointDev& pt = a.pts[p];
      const Fp4 q = f4::mul(f4::sub(rr, load4(&pt.rys)), load4(pt.inv + mine));
      ro = f4::add(ro, f4::mul(load4(&pt.apo), q));
    }
    store4(a.ro + mine, ro);
  }
}

__global__ __launch_bounds__(kBlock) void fold_kernel(const Fp4* v, const Fp4* add_in, Fp4* out, uint32_t log_rows,
                                                      const Fp4 half_beta, uint32_t half, const PowTable winv) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= (1u << log_rows)) return;
  // p_r = (beta / 2) w^-bitrev(r), w of order 2 rows
  const Fp4 pr = f4::mul_base(half_beta, pow_bits(winv, bitrev(r, log_rows), log_rows));
  Fp4 lo_f = pr, hi_f = f4::neg(pr);
  lo_f.c[0] = bb31::add(lo_f.c[0], half);
  hi_f.c[0] = bb31::add(hi_f.c[0], half);
  Fp4 s = f4::add(f4::mul(lo_f, load4(v + 2 * (size_t)r)), f4::mul(hi_f, load4(v + 2 * (size_t)r + 1)));
  if (add_in) s = f4::add(s, load4(add_in + r));
  store4(out + r, s);
}

// ---------------------------------------------------------------- host side

uint32_t root_mont(unsigned log_n) {  // w of order 2^log_n
  uint32_t r = bb31::kRootOfUnityMont;
  for (unsigned k = bb31::kTwoAdicity; k > log_n; --k) r = bb31::mul(r, r);
  return r;
}

PowTable make_table(uint32_t base) {
  PowTable t;
  for (unsigned j = 0; j <= kMaxLogRows; ++j) {
    t.w[j] = base;
    base = bb31::mul(base, base);
  }
  return t;
}

template <class Fn>
void with_point_group(unsigned n, Fn&& fn) {
  if (n <= 1) fn(std::integral_constant<int, 1>{});
  else if (n <= 2) fn(std::integral_constant<int, 2>{});
  else if (n <= 4) fn(std::integral_constant<int, 4>{});
  else fn(std::integral_constant<int, (int)kPointGroup>{});
}

}  // namespace

void bb4_ops(int op, const Fp4* d_a, const Fp4* d_b, Fp4* d_out, size_t count, hipStream_t stream) {
  if (count == 0) return;
  hipLaunchKernelGGL(ops_kernel, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, stream, op, d_a, d_b, d_out, count);
  TA_HIP(hipGetLastError());
}

FriOpening::FriOpening(unsigned log_blowup, int external, hipStream_t stream)
    : log_blowup_(log_blowup), external_(external), stream_(stream) {
  require_gpu();
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  phase_.log_blowup = log_blowup;
  flag_.ensure(sizeof(uint32_t));
}

FriOpening::~FriOpening() {
  (void)hipStreamSynchronize(stream_);
  trees_.clear();  // they wait for the stream themselves
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

bool FriOpening::begin(const Fp4& alpha) {
  for (int k = 0; k < 4; ++k)
    if (alpha.c[k] >= bb31::kP) return false;
  alpha_ = alpha;
  Phase p;
  p.begun = true;
  p.log_blowup = log_blowup_;
  phase_ = p;
  for (unsigned k = 0; k <= kMaxLogRows; ++k) {
    ro_present_[k] = false;
    num_reduced_[k] = 0;
  }
  inputs_.clear();
  inv_.clear();      // (freeing a buffer waits for the device; the buffers of ro_, folds_ and trees_ are reused)
  uploads_.clear();
  apow_count_ = 0;
  num_commits_ = 0;
  launches_ = 0;
  TA_HIP(hipMemsetAsync(flag_.as<void>(), 0, sizeof(uint32_t), stream_));
  return true;
}

void FriOpening::ensure_alpha_powers(size_t cols) {
  if (cols <= apow_count_) return;
  // (growing frees the old table, which waits for the kernels that read it)
  Fp4* out = static_cast<Fp4*>(apow_.ensure(cols * sizeof(Fp4)));
  hipLaunchKernelGGL(alpha_pow_kernel, dim3(ceil_div(cols, kBlock)), dim3(kBlock), 0, stream_, alpha_, (uint32_t)cols,
                     out);
  ++launches_;
  apow_count_ = cols;
}

const Fp4* FriOpening::inv_denoms(const Fp4& z, unsigned log_n) {
  InvDenoms* e = nullptr;
  for (InvDenoms& d : inv_)
    if (f4::equal(d.z, z)) e = &d;
  if (e && e->log_n >= log_n) return e->buf->as<Fp4>();
  if (!e) {
    inv_.push_back(InvDenoms{z, 0, nullptr});
    e = &inv_.back();
  } else {
    uploads_.push_back(std::move(e->buf));  // kernels in flight still read it
  }
  e->buf = std::make_unique<DeviceBuffer>();
  e->log_n = log_n;
  Fp4* out = static_cast<Fp4*>(e->buf->ensure((sizeof(Fp4)) << log_n));
  hipLaunchKernelGGL(inv_denoms_kernel, dim3(ceil_div(size_t(1) << log_n, kBlock)), dim3(kBlock), 0, stream_, z,
                     make_table(root_mont(log_n)), bb31::to_mont(bb31::kGenerator), (uint32_t)log_n, out,
                     flag_.as<uint32_t>());
  ++launches_;
  return out;
}

bool FriOpening::add_round(const void* const* ldes, const size_t* rows, const size_t* cols, size_t count,
                           const void* const* points, const size_t* num_points, void* const* opened_values_out) {
  if (!can_add_round(phase_) ||
      !round_ok(ldes, rows, cols, count, points, num_points, opened_values_out, log_blowup_))
    return false;
  size_t total_points = 0, total_ys = 0, max_cols = 0;
  for (size_t m = 0; m < count; ++m) {
    for (size_t p = 0; p < num_points[m]; ++p)
      for (int k = 0; k < 4; ++k)
        if (load_ext(points[m], p).c[k] >= bb31::kP) return false;
    total_points += num_points[m];
    total_ys += num_points[m] * cols[m];
    max_cols = std::max(max_cols, cols[m]);
  }
  launches_ = 0;

  // host matrices are uploaded; device matrices are used where they are
  std::vector<const uint32_t*> dev(count);
  for (size_t m = 0; m < count; ++m) {
    if (is_device_pointer(ldes[m])) {
      dev[m] = static_cast<const uint32_t*>(ldes[m]);
      continue;
    }
    const size_t bytes = rows[m] * cols[m] * sizeof(uint32_t);
    uploads_.push_back(std::make_unique<DeviceBuffer>());
    void* d = uploads_.back()->ensure(bytes);
    TA_HIP(hipMemcpyAsync(d, ldes[m], bytes, hipMemcpyHostToDevice, stream_));
    dev[m] = static_cast<const uint32_t*>(d);
  }

  ensure_alpha_powers(max_cols);
  const uint32_t g = bb31::to_mont(bb31::kGenerator);

  // the points' records: inverse denominators, alpha^offset and the
  // interpolation's scale, in the reference's order
  std::vector<PointDev> host_pts(total_points);
  std::vector<size_t> pts_at(count), ys_at(count);
  size_t at = 0, yat = 0;
  for (size_t m = 0; m < count; ++m) {
    const unsigned log_n = log2_exact(rows[m]), log_m = log_n - log_blowup_;
    pts_at[m] = at;
    ys_at[m] = yat;
    if (!ro_present_[log_n]) {
      if (!ro_[log_n]) ro_[log_n] = std::make_unique<DeviceBuffer>();
      void* d = ro_[log_n]->ensure(sizeof(Fp4) << log_n);
      TA_HIP(hipMemsetAsync(d, 0, sizeof(Fp4) << log_n, stream_));
      ro_present_[log_n] = true;
    }
    // m g^(m-1), the same for every point of the matrix
    const uint32_t mm = bb31::to_mont((uint32_t)(size_t(1) << log_m));
    const uint32_t denom_inv = bb31::inverse(bb31::mul(mm, bb31::pow(g, (size_t(1) << log_m) - 1)));
    const uint32_t gm = bb31::pow(g, size_t(1) << log_m);
    for (size_t p = 0; p < num_points[m]; ++p, ++at) {
      const Fp4 z = load_ext(points[m], p);
      PointDev& pt = host_pts[at];
      memset(&pt, 0, sizeof pt);
      pt.inv = inv_denoms(z, log_n);
      pt.apo = f4::pow(alpha_, num_reduced_[log_n]);
      num_reduced_[log_n] += cols[m];
      Fp4 zm = z;
      for (unsigned k = 0; k < log_m; ++k) zm = f4::square(zm);
      pt.scale = f4::mul_base(f4::sub(zm, f4::from_base(gm)), denom_inv);
    }
    yat += num_points[m] * cols[m];
  }
  PointDev* d_pts = static_cast<PointDev*>(pts_.ensure(std::max<size_t>(1, total_points) * sizeof(PointDev)));
  Fp4* d_ys = static_cast<Fp4*>(ys_.ensure(std::max<size_t>(1, total_ys) * sizeof(Fp4)));
  if (total_points)
    TA_HIP(hipMemcpyAsync(d_pts, host_pts.data(), total_points * sizeof(PointDev), hipMemcpyHostToDevice, stream_));

  for (size_t m = 0; m < count; ++m) {
    const unsigned log_n = log2_exact(rows[m]), log_m = log_n - log_blowup_;
    const size_t mrows = size_t(1) << log_m;
    const uint32_t ncols = (uint32_t)cols[m];
    const unsigned col_blocks = ceil_div(ncols, kInterpCols);
    // at most about kInterpBlocks blocks, each over a power-of-two run of at least two tiles of rows
    size_t rows_per_block = 2 * kInterpTile;
    while (rows_per_block < mrows && (mrows / rows_per_block) * col_blocks > kInterpBlocks) rows_per_block *= 2;
    const unsigned row_blocks = ceil_div(mrows, rows_per_block);
    const PowTable wm = make_table(root_mont(log_m));

    for (size_t p0 = 0; p0 < num_points[m]; p0 += kPointGroup) {
      const unsigned np = (unsigned)std::min<size_t>(kPointGroup, num_points[m] - p0);
      Fp4* partial = static_cast<Fp4*>(partial_.ensure((size_t)row_blocks * np * ncols * sizeof(Fp4)));
      InterpArgs ia{};
      ia.mat = dev[m];
      ia.cols = ncols;
      ia.log_m = log_m;
      ia.log_blowup = log_blowup_;
      ia.rows_per_block = (uint32_t)rows_per_block;
      ia.num_points = np;
      ia.pts = d_pts + pts_at[m] + p0;
      ia.wm = wm;
      ia.partial = partial;
      with_point_group(np, [&](auto pg) {
        hipLaunchKernelGGL(interp_kernel<decltype(pg)::value>, dim3(row_blocks, col_blocks), dim3(kBlock), 0, stream_,
                           ia);
      });
      Fp4* ys = d_ys + ys_at[m] + p0 * ncols;
      hipLaunchKernelGGL(finish_kernel, dim3(ceil_div(ncols, 16), np), dim3(kBlock), 0, stream_, partial, row_blocks,
                         np, ncols, d_pts + pts_at[m] + p0, ys);
      hipLaunchKernelGGL(reduced_ys_kernel, dim3(np), dim3(kBlock), 0, stream_, ys, ncols, apow_.as<Fp4>(),
                         d_pts + pts_at[m] + p0);
      launches_ += 3;
    }

    ReduceArgs ra{};
    ra.mat = dev[m];
    ra.cols = ncols;
    ra.log_n = log_n;
    ra.num_points = (uint32_t)num_points[m];
    ra.apow = apow_.as<Fp4>();
    ra.pts = d_pts + pts_at[m];
    ra.ro = ro_[log_n]->as<Fp4>();
    if (num_points[m]) {  // without points the height's vector only has to exist
      hipLaunchKernelGGL(reduce_kernel, dim3(ceil_div(rows[m], kTileRows)), dim3(kBlock), 0, stream_, ra);
      ++launches_;
    }
  }
  TA_HIP(hipGetLastError());

  uint32_t flag = 0;
  for (size_t m = 0; m < count; ++m)
    if (num_points[m])
      TA_HIP(hipMemcpyAsync(opened_values_out[m], d_ys + ys_at[m], num_points[m] * cols[m] * sizeof(Fp4),
                            hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipMemcpyAsync(&flag, flag_.as<void>(), sizeof flag, hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));

  inputs_.clear();
  for (int k = (int)kMaxLogRows; k >= 0; --k)
    if (ro_present_[k]) inputs_.push_back((unsigned)k);
  phase_.has_input = true;
  phase_.log_max = inputs_[0];
  if (flag) {
    phase_.poisoned = true;
    return false;
  }
  return true;
}

const Fp4* FriOpening::input_device(size_t k) const {
  return k < inputs_.size() ? ro_[inputs_[k]]->as<Fp4>() : nullptr;
}

bool FriOpening::input(size_t k, void* out) {
  if (!usable(phase_) || k >= inputs_.size() || !out) return false;
  TA_HIP(hipMemcpyAsync(out, input_device(k), sizeof(Fp4) << inputs_[k], hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
  return true;
}

const Fp4* FriOpening::folded(size_t i) const {
  return i == 0 ? ro_[phase_.log_max]->as<Fp4>() : folds_[i - 1]->as<Fp4>();
}

int FriOpening::commit(void* root_out) {
  if (!can_commit(phase_) || !root_out) return -1;
  const bool work = commit_has_work(phase_);
  if (!phase_.started) {
    phase_.started = true;
    phase_.log_size = phase_.log_max;
  }
  if (!work) return 0;
  if (trees_.size() <= num_commits_) trees_.push_back(std::make_unique<hash::BbMerkleTree>(external_, stream_));
  // the folded vector is its own leaf matrix: size / 2 rows of two elements
  const void* mat = folded(num_commits_);
  const size_t rows = size_t(1) << (phase_.log_size - 1), cols = 8;
  hash::BbMerkleTree& tree = *trees_[num_commits_];
  if (!tree.build(&mat, &rows, &cols, 1, 0) || !tree.root(root_out)) return -1;
  launches_ = tree.last_launches();
  ++num_commits_;
  phase_.pending = true;
  return 1;
}

bool FriOpening::fold(const Fp4& beta) {
  if (!can_fold(phase_)) return false;
  for (int k = 0; k < 4; ++k)
    if (beta.c[k] >= bb31::kP) return false;
  const size_t step = num_commits_ - 1;
  const unsigned log_rows = phase_.log_size - 1;
  if (folds_.size() <= step) folds_.push_back(std::make_unique<DeviceBuffer>());
  Fp4* out = static_cast<Fp4*>(folds_[step]->ensure(sizeof(Fp4) << log_rows));
  const Fp4* add_in = ro_present_[log_rows] ? ro_[log_rows]->as<Fp4>() : nullptr;
  const uint32_t half = bb31::inverse(bb31::to_mont(2));
  const uint32_t winv = bb31::inverse(root_mont(log_rows + 1));
  hipLaunchKernelGGL(fold_kernel, dim3(ceil_div(size_t(1) << log_rows, kBlock)), dim3(kBlock), 0, stream_,
                     folded(step), add_in, out, (uint32_t)log_rows, f4::mul_base(beta, half), half, make_table(winv));
  TA_HIP(hipGetLastError());
  launches_ = 1;
  phase_.log_size = log_rows;
  phase_.pending = false;
  return true;
}

bool FriOpening::final_poly(void* out) {
  if (!ended(phase_) || !out) return false;
  TA_HIP(hipMemcpyAsync(out, folded(num_commits_), sizeof(Fp4) << phase_.log_size, hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
  return true;
}

}  // namespace tachyon_amd::fri
