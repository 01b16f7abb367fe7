// BabyBear NTT passes for gfx950 (see ntt_bb.h for the plan).
#include "ntt_bb.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "../field/bb31.h"

namespace tachyon_amd::ntt {

namespace {

constexpr uint32_t kBbBlock = 1024;  // two workgroups per CU at the largest tile: 8 waves per SIMD
constexpr uint32_t kBbLogBlock = 10;
constexpr uint32_t kBbLogTile = 14;  // R * T <= 2^14 words of LDS (+ padding)

enum : uint32_t {
  kBbLoadCoset = 1,   // first pass: input row i times cs^i
  kBbStoreCoset = 2,  // last pass: output row K times cs^K
  kBbStoreScale = 4,  // last pass: output times scale
  kBbKFast = 8,       // s' = 1, m > 1: store with lanes along k (contiguous)
};

struct BbPassArgs {
  const uint32_t* in;
  uint32_t* out;
  const uint32_t* tw_lo;  // powers of g (forward) or g^-1 (inverse)
  const uint32_t* tw_hi;
  const uint32_t* cs_lo;  // powers of the coset factor
  const uint32_t* cs_hi;
  size_t bstride;       // words per batch item
  uint64_t V;           // batch * W virtual columns
  uint32_t W;           // m s': words per tile row = row stride
  uint32_t sp;          // s' = s C
  uint32_t C;           // columns
  uint32_t rows_valid;  // input rows at or above it read as zero
  uint32_t lb;          // bits of the lo tables
  uint32_t log_N;       // order of the tables
  uint32_t log_R;       // stages of this pass
  uint32_t log_ncur;    // log2(R m)
  uint32_t log_T;       // tile width
  uint32_t log_W;       // log2(W), kBbKFast only
  uint32_t flags;
  uint32_t scale;
};

__device__ __forceinline__ uint32_t pow2l(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                          uint32_t lb, uint32_t e) {
  return bb31::mul(lo[e & ((1u << lb) - 1)], hi[e >> lb]);
}

// One Stockham pass: tile of R rows x T words in LDS (row pitch T + 1), the
// R-point DFT as decimation in time on bit-reversed rows, two radix-2 stages
// per LDS round trip (one twiddle-free stage first when log R is odd).
__global__ __launch_bounds__(kBbBlock) void bb_pass_kernel(const BbPassArgs a) {
  extern __shared__ uint32_t bb_lds[];
  const uint32_t R = 1u << a.log_R, T = 1u << a.log_T, TP = T + 1;
  uint32_t* tile = bb_lds;
  uint32_t* wr = bb_lds + R * TP;  // w_R^i, i < R / 2
  const uint32_t tid = threadIdx.x;
  const uint32_t lm = a.log_ncur - a.log_R;

  for (uint32_t i = tid; i < (R >> 1); i += kBbBlock)
    wr[i] = pow2l(a.tw_lo, a.tw_hi, a.lb, i << (a.log_N - a.log_R));

  const uint32_t vt = tid & (T - 1), rg = tid >> a.log_T, rs = kBbBlock >> a.log_T;
  const uint64_t v0 = (uint64_t)blockIdx.x << a.log_T;
  const bool live = v0 + vt < a.V;
  uint32_t t = 0, u = 0, p = 0, qp = 0;
  if (live) {
    const uint32_t v = (uint32_t)(v0 + vt);
    t = v / a.W;
    u = v - t * a.W;
    p = u / a.sp;
    qp = u - p * a.sp;
  }

  if (live) {
    const uint32_t* src = a.in + (size_t)t * a.bstride + u;
    for (uint32_t r = rg; r < R; r += rs) {
      const uint32_t i = p + (r << lm);  // row of the sub-transform
      uint32_t x = 0;
      if (i < a.rows_valid) {
        x = src[(size_t)r * a.W];
        if (a.flags & kBbLoadCoset) x = bb31::mul(x, pow2l(a.cs_lo, a.cs_hi, a.lb, i));
      }
      tile[(__brev(r) >> (32 - a.log_R)) * TP + vt] = x;
    }
  } else {
    for (uint32_t r = rg; r < R; r += rs) tile[r * TP + vt] = 0;
  }
  __syncthreads();

  uint32_t lh = 0;
  if (a.log_R & 1) {
    // half 1: every twiddle is one
    const uint32_t nb = (R >> 1) << a.log_T;
    for (uint32_t b = tid; b < nb; b += kBbBlock) {
      const uint32_t col = b & (T - 1), jb = b >> a.log_T;
      const uint32_t i0 = (jb << 1) * TP + col, i1 = i0 + TP;
      const uint32_t x = tile[i0], y = tile[i1];
      tile[i0] = bb31::add(x, y);
      tile[i1] = bb31::sub(x, y);
    }
    lh = 1;
    __syncthreads();
  }
  const uint32_t nq = (R >> 2) << a.log_T;
  for (; lh < a.log_R; lh += 2) {
    // halves h and 2h on rows j, j + h, j + 2h, j + 3h
    const uint32_t h = 1u << lh;
    for (uint32_t b = tid; b < nq; b += kBbBlock) {
      const uint32_t col = b & (T - 1), jb = b >> a.log_T;
      const uint32_t jj = jb & (h - 1);
      const uint32_t j = ((jb >> lh) << (lh + 2)) | jj;
      const uint32_t w1 = wr[jj << (a.log_R - 1 - lh)];
      const uint32_t w2 = wr[jj << (a.log_R - 2 - lh)], w3 = wr[(jj + h) << (a.log_R - 2 - lh)];
      const uint32_t i0 = j * TP + col, i1 = i0 + h * TP, i2 = i1 + h * TP, i3 = i2 + h * TP;
      const uint32_t x0 = tile[i0], x1 = bb31::mul(tile[i1], w1);
      const uint32_t x2 = tile[i2], x3 = bb31::mul(tile[i3], w1);
      const uint32_t y0 = bb31::add(x0, x1), y1 = bb31::sub(x0, x1);
      const uint32_t y2 = bb31::mul(bb31::add(x2, x3), w2), y3 = bb31::mul(bb31::sub(x2, x3), w3);
      tile[i0] = bb31::add(y0, y2);
      tile[i2] = bb31::sub(y0, y2);
      tile[i1] = bb31::add(y1, y3);
      tile[i3] = bb31::sub(y1, y3);
    }
    __syncthreads();
  }

  const uint32_t tw_shift = a.log_N - a.log_ncur;
  if (a.flags & kBbKFast) {
    // s' = 1: output (k, p) at R p + k, lanes along k
    const uint32_t ne = R << a.log_T;
    for (uint32_t e = tid; e < ne; e += kBbBlock) {
      const uint32_t k = e & (R - 1), pl = e >> a.log_R;
      if (v0 + pl >= a.V) continue;
      const uint32_t v = (uint32_t)(v0 + pl);
      const uint32_t tt = v >> a.log_W, pp = v & (a.W - 1);
      const uint32_t x = bb31::mul(tile[k * TP + pl], pow2l(a.tw_lo, a.tw_hi, a.lb, (pp * k) << tw_shift));
      a.out[(size_t)tt * a.bstride + ((size_t)pp << a.log_R) + k] = x;
    }
  } else if (live) {
    uint32_t* dst = a.out + (size_t)t * a.bstride + qp + (size_t)a.sp * ((size_t)p << a.log_R);
    uint32_t q = 0, s = 0;
    if (a.flags & kBbStoreCoset) {
      q = qp / a.C;
      s = a.sp / a.C;
    }
    for (uint32_t k = rg; k < R; k += rs) {
      uint32_t x = tile[k * TP + vt];
      if (lm) x = bb31::mul(x, pow2l(a.tw_lo, a.tw_hi, a.lb, (p * k) << tw_shift));
      if (a.flags & kBbStoreCoset) x = bb31::mul(x, pow2l(a.cs_lo, a.cs_hi, a.lb, q + s * k));
      if (a.flags & kBbStoreScale) x = bb31::mul(x, a.scale);
      dst[(size_t)k * a.sp] = x;
    }
  }
}

// lo[i] = base^i (i < lo_cnt = 2^lb), hi[j] = base^(j 2^lb) (j < hi_cnt)
__global__ __launch_bounds__(kBbBlock) void bb_powers_kernel(uint32_t* lo, uint32_t* hi, uint32_t base, uint32_t lb,
                                                             uint32_t lo_cnt, uint32_t hi_cnt) {
  const uint32_t i = blockIdx.x * kBbBlock + threadIdx.x;
  if (i < lo_cnt) lo[i] = bb31::pow(base, i);
  else if (i - lo_cnt < hi_cnt) hi[i - lo_cnt] = bb31::pow(base, (uint64_t)(i - lo_cnt) << lb);
}

size_t bb_lds_bytes(uint32_t log_R, uint32_t log_T) {
  const size_t R = size_t(1) << log_R, T = size_t(1) << log_T;
  return (R * (T + 1) + (R >> 1)) * sizeof(uint32_t);
}

uint32_t ceil_log2(uint64_t x) {
  uint32_t l = 0;
  while ((uint64_t(1) << l) < x) ++l;
  return l;
}

}  // namespace

BbGenDomain::BbGenDomain(hipStream_t stream) : stream_(stream) {
  require_gpu();
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  const size_t max_lds = bb_lds_bytes(kMaxPassStages, kBbLogTile - kMaxPassStages);
  if (max_lds > 64 * 1024)
    TA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bb_pass_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds));
}

BbGenDomain::~BbGenDomain() {
  release();
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

std::vector<uint32_t> BbGenDomain::plan(uint32_t log_m) {
  const uint32_t passes = (log_m + kMaxPassStages - 1) / kMaxPassStages;
  std::vector<uint32_t> ks;
  for (uint32_t i = 0, left = log_m; i < passes; ++i) {
    const uint32_t k = (left + (passes - i) - 1) / (passes - i);
    ks.push_back(k);
    left -= k;
  }
  return ks;
}

void BbGenDomain::build_powers(Powers& t, uint32_t base) {
  const uint32_t lo_cnt = 1u << lb_, hi_cnt = 1u << (log_n_ - lb_);
  uint32_t* lo = static_cast<uint32_t*>(t.lo.ensure(lo_cnt * sizeof(uint32_t)));
  uint32_t* hi = static_cast<uint32_t*>(t.hi.ensure(hi_cnt * sizeof(uint32_t)));
  hipLaunchKernelGGL(bb_powers_kernel, dim3(ceil_div((size_t)lo_cnt + hi_cnt, kBbBlock)), dim3(kBbBlock), 0, stream_,
                     lo, hi, base, lb_, lo_cnt, hi_cnt);
  TA_HIP(hipGetLastError());
  t.base = base;
}

bool BbGenDomain::init(uint32_t group_gen) {
  if (inited_) return group_gen == gen_;
  if (group_gen >= bb31::kP) return false;
  // the order by repeated squaring: exactly 2^ln (0 never reaches one, an
  // element of another order not within the two-adicity)
  uint32_t ln = 0;
  for (uint32_t x = group_gen; x != bb31::kR; x = bb31::mul(x, x), ++ln)
    if (ln == kMaxLogOrder) return false;
  log_n_ = ln;
  lb_ = (ln + 1) / 2;
  gen_ = group_gen;
  // two-level twiddles, 2^lb + 2^(LN - lb) words per direction: any w_N^e is
  // one product, and no table grows with N / 2
  build_powers(fwd_, group_gen);
  build_powers(inv_, bb31::inverse(group_gen));
  TA_HIP(hipStreamSynchronize(stream_));
  inited_ = true;
  return true;
}

void BbGenDomain::release() {
  if (stream_) (void)hipStreamSynchronize(stream_);
  inited_ = false;
  log_n_ = lb_ = 0;
  gen_ = 0;
  tick_ = 0;
  for (Powers* t : {&fwd_, &inv_}) {
    t->lo.release();
    t->hi.release();
  }
  for (Powers& c : cosets_) {
    c.used = 0;
    c.lo.release();
    c.hi.release();
  }
  for (DeviceBuffer* b : {&scratch_, &lde_, &io_, &io2_}) b->release();
}

size_t BbGenDomain::table_bytes() const {
  if (!inited_) return 0;
  size_t bytes = fwd_.lo.capacity() + fwd_.hi.capacity() + inv_.lo.capacity() + inv_.hi.capacity();
  for (const Powers& c : cosets_) bytes += c.lo.capacity() + c.hi.capacity();
  return bytes;
}

// The power tables of `base`: the cached entry, or the least recently used one
// rebuilt on the device behind the passes that still read its old values.
const BbGenDomain::Powers& BbGenDomain::powers(uint32_t base) {
  Powers* victim = &cosets_[0];
  for (Powers& c : cosets_) {
    if (c.used && c.base == base) {
      c.used = ++tick_;
      return c;
    }
    if (c.used < victim->used) victim = &c;
  }
  build_powers(*victim, base);
  victim->used = ++tick_;
  return *victim;
}

void BbGenDomain::transform(const uint32_t* src, uint32_t* dst, uint32_t* tmp, uint32_t log_n, uint32_t cols,
                            uint32_t batch, bool inverse, const Powers* load_cs, const Powers* store_cs, bool scale,
                            uint32_t rows_valid) {
  const std::vector<uint32_t> ks = plan(log_n);
  const Powers& tw = inverse ? inv_ : fwd_;
  const size_t bstride = ((size_t)cols) << log_n;
  uint32_t log_ncur = log_n;
  const uint32_t* in = src;
  for (size_t i = 0; i < ks.size(); ++i) {
    const bool first = i == 0, last = i + 1 == ks.size();
    const uint32_t log_R = ks[i];
    const uint32_t log_s = log_n - log_ncur, lm = log_ncur - log_R;
    BbPassArgs a{};
    a.in = in;
    a.out = (first && !last) ? tmp : dst;
    a.tw_lo = tw.lo.as<uint32_t>();
    a.tw_hi = tw.hi.as<uint32_t>();
    a.bstride = bstride;
    a.sp = cols << log_s;
    a.W = a.sp << lm;
    a.V = (uint64_t)batch * a.W;
    a.C = cols;
    a.rows_valid = first ? rows_valid : 0xffffffffu;
    a.lb = lb_;
    a.log_N = log_n_;
    a.log_R = log_R;
    a.log_ncur = log_ncur;
    a.log_T = std::min<uint32_t>(std::min(kBbLogBlock, kBbLogTile - log_R), ceil_log2(a.V));
    a.flags = 0;
    if (first && load_cs) {
      a.flags |= kBbLoadCoset;
      a.cs_lo = load_cs->lo.as<uint32_t>();
      a.cs_hi = load_cs->hi.as<uint32_t>();
    }
    if (last && store_cs) {
      a.flags |= kBbStoreCoset;
      a.cs_lo = store_cs->lo.as<uint32_t>();
      a.cs_hi = store_cs->hi.as<uint32_t>();
    }
    if (last && scale) {
      a.flags |= kBbStoreScale;
      a.scale = bb31::inverse(bb31::to_mont(1u << log_n));
    }
    if (a.sp == 1 && lm > 0) {
      a.flags |= kBbKFast;
      a.log_W = lm;
    }
    const uint64_t blocks = (a.V + (uint64_t(1) << a.log_T) - 1) >> a.log_T;
    hipLaunchKernelGGL(bb_pass_kernel, dim3((unsigned)blocks), dim3(kBbBlock), bb_lds_bytes(log_R, a.log_T), stream_,
                       a);
    ++launches_;
    in = a.out;
    log_ncur -= log_R;
  }
  TA_HIP(hipGetLastError());
}

void BbGenDomain::run(uint32_t* d_data, uint32_t log_m, bool inverse, size_t batch, uint32_t coset) {
  if (!inited_) throw std::runtime_error("tachyon_mi355x: NTT run before init");
  if (log_m > log_n_) throw std::runtime_error("tachyon_mi355x: NTT size above the initialised domain");
  launches_ = 0;
  // size 1: forward is the identity (h^0 = 1); inverse scales by 1^-1
  if (log_m == 0 || batch == 0) return;
  if ((batch << log_m) >> 32) throw std::runtime_error("tachyon_mi355x: NTT batch exceeds 32-bit indexing");
  uint32_t* tmp = plan(log_m).size() > 1 ? static_cast<uint32_t*>(scratch_.ensure((batch << log_m) * 4)) : nullptr;
  const bool plain = coset == bb31::kR;
  if (inverse)
    transform(d_data, d_data, tmp, log_m, 1, (uint32_t)batch, true, nullptr,
              plain ? nullptr : &powers(bb31::inverse(coset)), true, 0xffffffffu);
  else
    transform(d_data, d_data, tmp, log_m, 1, (uint32_t)batch, false, plain ? nullptr : &powers(coset), nullptr, false,
              0xffffffffu);
}

void BbGenDomain::run_host(uint32_t* data, uint32_t log_m, bool inverse, size_t batch, uint32_t coset) {
  const size_t bytes = (batch << log_m) * sizeof(uint32_t);
  uint32_t* d = static_cast<uint32_t*>(io_.ensure(bytes));
  TA_HIP(hipMemcpyAsync(d, data, bytes, hipMemcpyHostToDevice, stream_));
  run(d, log_m, inverse, batch, coset);
  TA_HIP(hipMemcpyAsync(data, d, bytes, hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

void BbGenDomain::run_columns(uint32_t* d_mat, uint32_t log_rows, size_t cols, bool inverse, uint32_t coset) {
  if (!inited_) throw std::runtime_error("tachyon_mi355x: NTT run before init");
  if (log_rows > log_n_) throw std::runtime_error("tachyon_mi355x: NTT size above the initialised domain");
  launches_ = 0;
  if (log_rows == 0 || cols == 0) return;
  if ((cols << log_rows) >> 32) throw std::runtime_error("tachyon_mi355x: NTT matrix exceeds 32-bit indexing");
  uint32_t* tmp =
      plan(log_rows).size() > 1 ? static_cast<uint32_t*>(scratch_.ensure((cols << log_rows) * 4)) : nullptr;
  const bool plain = coset == bb31::kR;
  if (inverse)
    transform(d_mat, d_mat, tmp, log_rows, (uint32_t)cols, 1, true, nullptr,
              plain ? nullptr : &powers(bb31::inverse(coset)), true, 0xffffffffu);
  else
    transform(d_mat, d_mat, tmp, log_rows, (uint32_t)cols, 1, false, plain ? nullptr : &powers(coset), nullptr, false,
              0xffffffffu);
}

void BbGenDomain::run_columns_host(uint32_t* mat, uint32_t log_rows, size_t cols, bool inverse, uint32_t coset) {
  const size_t bytes = (cols << log_rows) * sizeof(uint32_t);
  uint32_t* d = static_cast<uint32_t*>(io_.ensure(bytes));
  TA_HIP(hipMemcpyAsync(d, mat, bytes, hipMemcpyHostToDevice, stream_));
  run_columns(d, log_rows, cols, inverse, coset);
  TA_HIP(hipMemcpyAsync(mat, d, bytes, hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

void BbGenDomain::coset_lde(const uint32_t* d_in, uint32_t log_rows, size_t cols, uint32_t added_bits, uint32_t shift,
                            uint32_t* d_out) {
  if (!inited_) throw std::runtime_error("tachyon_mi355x: NTT run before init");
  const uint32_t log_out = log_rows + added_bits;
  if (log_out > log_n_) throw std::runtime_error("tachyon_mi355x: LDE size above the initialised domain");
  if (cols == 0 || ((cols << log_out) >> 32))
    throw std::runtime_error("tachyon_mi355x: LDE matrix exceeds 32-bit indexing");
  launches_ = 0;
  const size_t in_words = cols << log_rows, out_words = cols << log_out;
  // coefficients (compact, rows x cols) and the passes' ping-pong buffer
  uint32_t* coeffs = static_cast<uint32_t*>(lde_.ensure(in_words * 4));
  uint32_t* tmp = static_cast<uint32_t*>(scratch_.ensure(out_words * 4));
  if (log_rows == 0) {
    // one row: the interpolant is the constant, shift^0 / 1 = 1
    TA_HIP(hipMemcpyAsync(coeffs, d_in, in_words * 4, hipMemcpyDeviceToDevice, stream_));
  } else {
    // inverse on the plain domain; its last pass stores coefficient j times shift^j / rows
    transform(d_in, coeffs, tmp, log_rows, (uint32_t)cols, 1, true, nullptr, &powers(shift), true, 0xffffffffu);
  }
  if (log_out == 0) {
    TA_HIP(hipMemcpyAsync(d_out, coeffs, in_words * 4, hipMemcpyDeviceToDevice, stream_));
    return;
  }
  // forward at rows << added_bits; its first pass reads the missing rows as zero
  transform(coeffs, d_out, tmp, log_out, (uint32_t)cols, 1, false, nullptr, nullptr, false, 1u << log_rows);
}

void BbGenDomain::coset_lde_host(const uint32_t* in, uint32_t log_rows, size_t cols, uint32_t added_bits,
                                 uint32_t shift, uint32_t* out) {
  const size_t in_bytes = (cols << log_rows) * 4, out_bytes = in_bytes << added_bits;
  uint32_t* d_in = static_cast<uint32_t*>(io_.ensure(in_bytes));
  uint32_t* d_out = static_cast<uint32_t*>(io2_.ensure(out_bytes));
  TA_HIP(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, stream_));
  coset_lde(d_in, log_rows, cols, added_bits, shift, d_out);
  TA_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

}  // namespace tachyon_amd::ntt
