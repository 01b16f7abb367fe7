// The NTT's table and layout kernels: the stage tables and their Shoup form,
// the four-step's exchange table, transposes and unfused exchange, and the
// coset power tables.  Device code of ntt.hip's translation unit: included
// there only, after ntt_pass32.h and ntt_pass29.h.
#pragma once
#include "ntt_pass29.h"

namespace tachyon_amd::ntt {

namespace {

// T0[j] = w^j for j < n/2 from two small power tables: lo[j & mask] * hi[j >> bits]
template <class Fr>
__global__ __launch_bounds__(kBlock) void twiddle_base_kernel(Fr* __restrict__ t0, uint32_t count,
                                                              const Fr* __restrict__ lo, const Fr* __restrict__ hi,
                                                              uint32_t bits) {
  uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= count) return;
  t0[j] = (lo[j & ((1u << bits) - 1)] * hi[j >> bits]).canonical();  // canonical: see radix_step
}

// Montgomery twiddle table -> Shoup entries {plain w, floor(w 2^256 / p)}
template <class Fr>
__global__ __launch_bounds__(kBlock) void shoup_table_kernel(ShoupTw<Fr>* __restrict__ out,
                                                             const Fr* __restrict__ in, uint32_t count) {
  uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= count) return;
  const Fr w = in[j].from_mont();
  out[j] = ShoupTw<Fr>{w, Fr::shoup_quotient(w)};
}

// T_s[j] = T_0[j << s]  (the strided sub-sampling of radix2_twiddle_cache.h:105-117)
template <class T>
__global__ __launch_bounds__(kBlock) void twiddle_stage_kernel(T* __restrict__ ts, const T* __restrict__ t0,
                                                               uint32_t count, uint32_t s) {
  uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= count) return;
  ts[j] = t0[(size_t)j << s];
}

// FourStepTw::tab29: entry (c_l << log_r) + k1 = w_N^((c0 + c_l) k1) of this
// rank (the direction's power tables in f) in R'-form (32 W mod p, W the
// canonical Montgomery value: five doublings, as tw29_table_kernel)
__global__ __launch_bounds__(kBlock) void fs_table29_kernel(FourStepTw<Bn254Fr> f, uint32_t log_r, size_t count,
                                                            fr29::TwMont29* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= count) return;
  const uint32_t c_l = (uint32_t)(j >> log_r), k1 = (uint32_t)(j & ((size_t(1) << log_r) - 1));
  Bn254Fr x = fs_twiddle(f, k1, c_l).canonical();
#pragma unroll
  for (int i = 0; i < 5; ++i) x = (x + x).canonical();
  out[j].w = fr29::from_words(x.v);
}

// out[c][r] = in[r][c] for a rows x cols row-major matrix, through 32 x 32 LDS tiles
template <class Fr>
__global__ __launch_bounds__(kBlock) void transpose_kernel(const Fr* __restrict__ in, Fr* __restrict__ out,
                                                           uint32_t rows, uint32_t cols) {
  __shared__ Fr tile[32][33];
  const uint32_t c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (uint32_t j = ty; j < 32; j += 8) {
    const uint32_t r = r0 + j, c = c0 + tx;
    if (r < rows && c < cols) tile[j][tx] = in[(size_t)r * cols + c];
  }
  __syncthreads();
  for (uint32_t j = ty; j < 32; j += 8) {
    const uint32_t c = c0 + j, r = r0 + tx;
    if (r < rows && c < cols) out[(size_t)c * rows + r] = tile[tx][j];
  }
}

// forward: send[(h * Cg + c_l) * Rg + k1_l] = work[c_l * R + k1] * w^((c0 + c_l) k1), k1 = h Rg + k1_l
// inverse (unpack = true): out[c_l * R + k1] = recv[(h * Cg + c_l) * Rg + k1_l] * w^-((c0 + c_l) k1)
template <class Fr>
__global__ __launch_bounds__(kBlock) void twiddle_exchange_kernel(const Fr* __restrict__ in, Fr* __restrict__ out,
                                                                  uint32_t log_r, uint32_t log_rg, uint32_t log_cg,
                                                                  uint32_t c0, uint32_t log_n, const Fr* __restrict__ lo,
                                                                  const Fr* __restrict__ hi, uint32_t pow_bits,
                                                                  uint32_t unpack) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;  // position in the [c_l][k1] view
  if (i >= ((size_t)1 << (log_cg + log_r))) return;
  const uint32_t c_l = (uint32_t)(i >> log_r), k1 = (uint32_t)(i & ((1u << log_r) - 1));
  const uint32_t h = k1 >> log_rg, k1_l = k1 & ((1u << log_rg) - 1);
  const size_t j = (((size_t)h << log_cg) + c_l) * ((size_t)1 << log_rg) + k1_l;  // packed position
  const uint64_t e = ((uint64_t)(c0 + c_l) * k1) & ((uint64_t(1) << log_n) - 1);
  const Fr w = lo[e & ((1u << pow_bits) - 1)] * hi[e >> pow_bits];
  if (!unpack) out[j] = in[i] * w;
  else out[i] = in[j] * w;
}

// The two-level power tables of a coset offset, built on the device (no host
// vector, copy or synchronisation): thread i < lo_cnt writes lo[i] = scale
// base^i, thread lo_cnt + j writes hi[j] = base^(j 2^bits) (j < hi_cnt), each
// by square-and-multiply over its exponent (< 2^30).  Canonical values -- the
// field elements NttDomain::build_powers uploads.
template <class Fr>
__global__ __launch_bounds__(kBlock) void coset_powers_kernel(Fr* __restrict__ lo, Fr* __restrict__ hi, Fr base,
                                                              Fr scale, uint32_t bits, uint32_t lo_cnt,
                                                              uint32_t hi_cnt) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= lo_cnt + hi_cnt) return;
  const bool high = t >= lo_cnt;
  uint32_t e = high ? (t - lo_cnt) << bits : t;
  Fr acc = high ? Fr::one() : scale;
  Fr b = base;
  while (e) {
    if (e & 1) acc = acc * b;
    e >>= 1;
    if (e) b = b.sqr();
  }
  if (high) hi[t - lo_cnt] = acc.canonical();
  else lo[t] = acc.canonical();
}

}  // namespace

}  // namespace tachyon_amd::ntt
