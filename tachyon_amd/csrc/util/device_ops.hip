// Device helpers around the hot path:
//  * synthetic MSM inputs generated on the GPU (the bench needs 2^26 points in
//    HBM; the scheme mirrors test/random.h:12-28 and big_int.h:107-115, and is
//    bit-identical to the oracle's generator so tests can cross-check it);
//  * elementwise field / point parity kernels (the reference's
//    prime_field_correctness_gpu_test.cc and *_point_correctness_gpu_test.cc);
//  * the same for the carry-free limb fields of the hot kernels, on raw limbs
//    (tests/test_gpu_limb_fields.py).
#include "device_ops.h"

#include "../common/hip_util.h"
#include "../field/curve_constants.h"
#include "../field/f28.h"
#include "../field/f29.h"
#include "../field/fr29.h"
#include "../msm/acc28.h"
#include "../msm/acc29.h"
#include "../msm/pair28.h"
#include "../msm/pair29.h"

#include <utility>

namespace tachyon_amd::util {

namespace {

constexpr unsigned kBlock = 256;
constexpr uint64_t kGamma = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kBaseSeedXor = 0xBA5E5EEDBA5E5EEDull;

__device__ __forceinline__ uint64_t sm_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t rand_u64(uint64_t seed, uint64_t ctr) { return sm_mix(seed + (ctr + 1) * kGamma); }

// canonical 4-limb scalar below the modulus of Fr (BigInt<4>::Random semantics)
template <class Fr>
__device__ void rand_scalar(uint64_t seed, uint64_t i, uint64_t out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = rand_u64(seed, i * 4 + k);
  const uint64_t* m = Fr::Config::kP64;
  for (;;) {
    bool ge = true;
    for (int k = 3; k >= 0; --k) {
      if (out[k] != m[k]) { ge = out[k] > m[k]; break; }
    }
    if (!ge) break;
    for (int k = 0; k < 3; ++k) out[k] = (out[k] >> 1) | (out[k + 1] << 63);
    out[3] >>= 1;
  }
}

template <class Fr>
__device__ Fr limbs_to_fr(const uint64_t c[4]) {
  Fr x;
  for (int k = 0; k < 4; ++k) {
    x.v[2 * k] = (uint32_t)c[k];
    x.v[2 * k + 1] = (uint32_t)(c[k] >> 32);
  }
  return x;
}

template <class Fr>
__global__ __launch_bounds__(kBlock) void gen_scalars_kernel(uint64_t seed, uint64_t start, uint64_t n, Fr* out) {
  uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t c[4];
  rand_scalar<Fr>(seed, start + i, c);
  out[i] = limbs_to_fr<Fr>(c).to_mont().canonical();
}

template <class F>
__host__ __device__ F load_generator_coord(const uint64_t* src) {
  F r;
  uint32_t* dst = reinterpret_cast<uint32_t*>(&r);
  for (size_t i = 0; i < sizeof(F) / 4; ++i) dst[i] = (uint32_t)(src[i / 2] >> (32 * (i & 1)));
  return r;
}

template <class Curve>
struct Gen;
template <>
struct Gen<Bn254G1> {
  static constexpr const uint64_t* x() { return consts::bn254_g1::kXMont64; }
  static constexpr const uint64_t* y() { return consts::bn254_g1::kYMont64; }
};
template <>
struct Gen<Bn254G2> {
  static constexpr const uint64_t* x() { return consts::bn254_g2::kXMont64; }
  static constexpr const uint64_t* y() { return consts::bn254_g2::kYMont64; }
};
template <>
struct Gen<Bls381G1> {
  static constexpr const uint64_t* x() { return consts::bls12_381_g1::kXMont64; }
  static constexpr const uint64_t* y() { return consts::bls12_381_g1::kYMont64; }
};
template <>
struct Gen<Bls381G2> {
  static constexpr const uint64_t* x() { return consts::bls12_381_g2::kXMont64; }
  static constexpr const uint64_t* y() { return consts::bls12_381_g2::kYMont64; }
};

// One thread per chunk: k_j * G by double-and-add, then a doubling chain,
// each point normalised to affine (per-point inversion; a one-off setup cost).
// The call writes the global points [start, start + n): chunk j of the call is
// global chunk chunk0 + j, and the first one skips the (start - chunk0 * chunk)
// points before `start` with doublings, so any start gives the same sequence.
template <class Curve>
__global__ __launch_bounds__(kBlock) void gen_bases_kernel(uint64_t seed, uint64_t start, uint64_t n, uint64_t chunk,
                                                           uint64_t chunk0, Affine<typename Curve::F>* out) {
  using F = typename Curve::F;
  using Fr = typename Curve::Fr;
  uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t gbeg = (chunk0 + j) * chunk;  // global index of this chunk's first point
  const uint64_t lo = max(gbeg, start), hi = min(gbeg + chunk, start + n);
  if (lo >= hi) return;
  Affine<F> G{load_generator_coord<F>(Gen<Curve>::x()), load_generator_coord<F>(Gen<Curve>::y())};
  uint64_t k[4];
  rand_scalar<Fr>(seed ^ kBaseSeedXor, chunk0 + j, k);
  XYZZ<F> r = XYZZ<F>::zero();
  for (int limb = 3; limb >= 0; --limb)
    for (int bit = 63; bit >= 0; --bit) {
      r = r.dbl();
      if ((k[limb] >> bit) & 1) r = r.madd(G);
    }
  for (uint64_t i = gbeg; i < lo; ++i) r = r.dbl();
  for (uint64_t i = lo; i < hi; ++i) {
    out[i - start] = r.to_affine();
    r = r.dbl();
  }
}

template <class F>
__global__ __launch_bounds__(kBlock) void field_op_kernel(int op, const F* a, const F* b, F* out, size_t count) {
  size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  F x = a[i], y = b[i], r;
  switch (op) {
    case 0: r = x + y; break;
    case 1: r = x - y; break;
    case 2: r = x * y; break;
    case 3: r = x.sqr(); break;
    case 4: r = -x; break;
    case 5: r = x.inverse(); break;
    case 6: r = x.to_mont(); break;
    case 7: r = x.from_mont(); break;
    case 8: r = x.dbl(); break;
    case 9:  // x (any value < 2^(32N)) times the plain canonical constant y
      if constexpr (F::N == 8 && F::kLazyCapable) r = x.mul_shoup(y, F::shoup_quotient(y));
      else r = x * y.to_mont();
      break;
    // x y - y x (zero) and x y - x^2 through the fused a b - c d, in the hot
    // kernels' inline view (12-limb fields fuse only there)
    case 10: r = HotFp<F>(x).mul_sub(HotFp<F>(y), HotFp<F>(y), HotFp<F>(x)); break;
    case 11: r = HotFp<F>(x).mul_sub(HotFp<F>(y), HotFp<F>(x), HotFp<F>(x)); break;
    default: r = F::zero();
  }
  out[i] = r.canonical();
}

template <class F>
__global__ __launch_bounds__(kBlock) void ec_op_kernel(int op, const Affine<F>* a, const Affine<F>* b, Affine<F>* out,
                                                       size_t count) {
  size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  XYZZ<F> p = XYZZ<F>::from_affine(a[i]);
  XYZZ<F> r;
  switch (op) {
    case 0: r = p + XYZZ<F>::from_affine(b[i]); break;
    case 1: r = p.dbl(); break;
    case 2: r = p.madd(b[i]); break;
    default: r = XYZZ<F>::zero();
  }
  out[i] = r.to_affine();
}

template <class F>
void run_field_op(int op, const void* a, const void* b, void* out, size_t count) {
  if (count == 0) return;
  DeviceBuffer da, db, dout;
  size_t bytes = count * sizeof(F);
  TA_HIP(hipMemcpy(da.ensure(bytes), a, bytes, hipMemcpyHostToDevice));
  TA_HIP(hipMemcpy(db.ensure(bytes), b, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(field_op_kernel<F>, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, 0, op, da.as<F>(),
                     db.as<F>(), static_cast<F*>(dout.ensure(bytes)), count);
  TA_HIP(hipGetLastError());
  TA_HIP(hipMemcpy(out, dout.as<F>(), bytes, hipMemcpyDeviceToHost));
}

// RationalField<F>::BatchEvaluate (math/base/rational_field.h:51-76):
// out[i] = num[i] / den[i], with MultiplicativeGroup::DoBatchInverse's rule for
// a zero denominator (groups.h:124-180: its inverse is 0, so out[i] = 0).
// Montgomery's trick per thread over `chunk` consecutive elements: prefix
// products of the non-zero denominators go to `prefix`, one Fermat inverse
// per chunk, then the backward pass.  Results are canonical, so any chunking
// gives the reference's bytes.
template <class F>
__global__ __launch_bounds__(kBlock) void batch_evaluate_kernel(const F* __restrict__ num, const F* __restrict__ den,
                                                                F* __restrict__ out, F* __restrict__ prefix, size_t n,
                                                                uint32_t chunk) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t s = t * chunk;
  if (s >= n) return;
  const size_t e = s + chunk < n ? s + chunk : n;
  F prod = F::one();
  for (size_t i = s; i < e; ++i) {
    const F d = den[i];
    if (!d.is_zero()) prod = prod * d;
    prefix[i] = prod;
  }
  F inv = prod.inverse();  // product of non-zero values: invertible
  for (size_t i = e; i-- > s;) {
    const F d = den[i];
    if (d.is_zero()) {
      out[i] = F::zero();
      continue;
    }
    const F before = i > s ? prefix[i - 1] : F::one();  // product of the non-zero den[s..i)
    out[i] = (num[i] * (inv * before)).canonical();
    inv = inv * d;
  }
}

template <class F>
void run_ec_op(int op, const void* a, const void* b, void* out, size_t count) {
  if (count == 0) return;
  DeviceBuffer da, db, dout;
  size_t bytes = count * sizeof(Affine<F>);
  TA_HIP(hipMemcpy(da.ensure(bytes), a, bytes, hipMemcpyHostToDevice));
  TA_HIP(hipMemcpy(db.ensure(bytes), b, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(ec_op_kernel<F>, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, 0, op, da.as<Affine<F>>(),
                     db.as<Affine<F>>(), static_cast<Affine<F>*>(dout.ensure(bytes)), count);
  TA_HIP(hipGetLastError());
  TA_HIP(hipMemcpy(out, dout.as<Affine<F>>(), bytes, hipMemcpyDeviceToHost));
}

// ---- the limb fields of the hot kernels on raw limbs (tachyon_mi355x_limb_op) ----
// One kernel per (family, op): the op is a template parameter, the body is the
// inline function the hot kernels call, operands and results are raw limbs.
// Lane-pair ops (msm/pair29.h, pair28.h) take two adjacent lanes per element
// with a pair-uniform bounds check, so the DPP partner reads are defined.
struct LimbShape {
  int in = 0, out = 0;  // 32-bit words per element (in == 0: no such op)
  bool pair = false;
};

template <class F>
__device__ __forceinline__ F ld_limbs(const uint32_t* p) {
  F r;
#pragma unroll
  for (size_t i = 0; i < sizeof(F) / 4; ++i) r.l[i] = p[i];
  return r;
}
template <class F>
__device__ __forceinline__ void st_limbs(uint32_t* p, const F& x) {
#pragma unroll
  for (size_t i = 0; i < sizeof(F) / 4; ++i) p[i] = x.l[i];
}

// what differs between the two Fq limb fields: names and the site constants
// the lane-pair formulas instantiate their products with
struct Limb29 {
  using F = f29::F29;
  using Acc = msm::acc29_core::Acc;
  using PAcc = msm::pair29::Acc;
  static constexpr int N = 9, kWords = 8;
  static __device__ __forceinline__ F reduce(const F& v) { return f29::reduce_shl5(v); }
  static __device__ __forceinline__ F from32(const uint32_t* w) { return f29::from32(w); }
  static __device__ __forceinline__ F mul2_add5(const F& a, const F& b, const F& c, const F& d, const F& e) {
#if defined(__HIP_DEVICE_COMPILE__)
    return f29::asm29::mul2_add(a, b, c, d, e);
#else
    return f29::redc<true, true>(a, b, c, d, e);
#endif
  }
  static __device__ __forceinline__ Acc from_shifted(const F& x, const F& y) { return msm::acc29_core::from_shifted(x, y); }
  static __device__ __forceinline__ Acc madd(const Acc& a, const F& x, const F& y, int* sp) { return msm::acc29_core::madd(a, x, y, sp); }
  static __device__ __forceinline__ Acc add(const Acc& a, const Acc& b, int* sp) { return msm::acc29_core::add(a, b, sp); }
  static __device__ __forceinline__ Acc dbl(const Acc& a) { return msm::acc29_core::dbl(a); }
  static __device__ __forceinline__ bool pzero(const F& a) { return msm::pair29::pzero(a); }
  static __device__ __forceinline__ PAcc pfrom_shifted(const F& x, const F& y, bool h) { return msm::pair29::from_shifted(x, y, h); }
  static __device__ __forceinline__ PAcc pmadd(const PAcc& a, const F& x, const F& y, bool h, int* sp) { return msm::pair29::madd(a, x, y, h, sp); }
  static __device__ __forceinline__ PAcc padd(const PAcc& a, const PAcc& b, bool h, int* sp) { return msm::pair29::add(a, b, h, sp); }
  static __device__ __forceinline__ PAcc pdbl(const PAcc& a, bool h) { return msm::pair29::dbl(a, h); }
  // (kind, k) of msm/pair29.h's madd, add and dbl; k: 0 kK4 2 kK16 4 kK32r3 5 kK8r1
  static constexpr bool has_pair(int kind, int k) {
    return (kind == 0 && (k == 0 || k == 2)) || (kind == 1 && (k == 0 || k == 4)) || (kind == 2 && (k == 0 || k == 5)) ||
           (kind == 3 && k == 0);
  }
  template <int kKind, int kK>
  static __device__ __forceinline__ F pair_product(const F& a, const F& b, const F& e, bool h) {
    namespace p = msm::pair29;
    if constexpr (kKind == 0 && kK == 0) return p::pmul<f29::kK4>(a, b, h);
    else if constexpr (kKind == 0 && kK == 2) return p::pmul<f29::kK16>(a, b, h);
    else if constexpr (kKind == 1 && kK == 0) return p::pmul_add<f29::kK4>(a, b, e, h);
    else if constexpr (kKind == 1 && kK == 4) return p::pmul_add<f29::kK32r3>(a, b, e, h);
    else if constexpr (kKind == 2 && kK == 0) return p::psqr<f29::kK4>(a, h);
    else if constexpr (kKind == 2 && kK == 5) return p::psqr<f29::kK8r1>(a, h);
    else return p::psqr_add<f29::kK4>(a, e, h);
  }
};

struct Limb28 {
  using F = f28::F28;
  using Acc = msm::acc28_core::Acc;
  using PAcc = msm::pair28::Acc;
  static constexpr int N = 14, kWords = 12;
  static __device__ __forceinline__ F reduce(const F& v) { return f28::reduce(v); }
  static __device__ __forceinline__ F from32(const uint32_t* w) { return f28::from32(w); }
  static __device__ __forceinline__ F mul2_add5(const F& a, const F& b, const F& c, const F& d, const F& e) {
#if defined(__HIP_DEVICE_COMPILE__)
    return f28::asm28::mul2_add(a, b, c, d, e);
#else
    return f28::redc<true, true>(a, b, c, d, e);
#endif
  }
  static __device__ __forceinline__ Acc from_shifted(const F& x, const F& y) { return msm::acc28_core::from_shifted(x, y); }
  static __device__ __forceinline__ Acc madd(const Acc& a, const F& x, const F& y, int* sp) { return msm::acc28_core::madd(a, x, y, sp); }
  static __device__ __forceinline__ Acc add(const Acc& a, const Acc& b, int* sp) { return msm::acc28_core::add(a, b, sp); }
  static __device__ __forceinline__ Acc dbl(const Acc& a) { return msm::acc28_core::dbl(a); }
  static __device__ __forceinline__ bool pzero(const F& a) { return msm::pair28::pzero(a); }
  static __device__ __forceinline__ PAcc pfrom_shifted(const F& x, const F& y, bool h) { return msm::pair28::from_shifted(x, y, h); }
  static __device__ __forceinline__ PAcc pmadd(const PAcc& a, const F& x, const F& y, bool h, int* sp) { return msm::pair28::madd(a, x, y, h, sp); }
  static __device__ __forceinline__ PAcc padd(const PAcc& a, const PAcc& b, bool h, int* sp) { return msm::pair28::add(a, b, h, sp); }
  static __device__ __forceinline__ PAcc pdbl(const PAcc& a, bool h) { return msm::pair28::dbl(a, h); }
  // (kind, k) of msm/pair28.h's madd, add and dbl; k: 0 kK4 1 kK8 2 kK16 3 kK32 4 kK32r3
  static constexpr bool has_pair(int kind, int k) {
    return (kind == 0 && (k == 0 || k == 1 || k == 3)) || (kind == 1 && (k == 0 || k == 4)) ||
           (kind == 2 && (k == 2 || k == 3)) || (kind == 3 && (k == 0 || k == 2));
  }
  template <int kKind, int kK>
  static __device__ __forceinline__ F pair_product(const F& a, const F& b, const F& e, bool h) {
    namespace p = msm::pair28;
    if constexpr (kKind == 0 && kK == 0) return p::pmul<f28::kK4>(a, b, h);
    else if constexpr (kKind == 0 && kK == 1) return p::pmul<f28::kK8>(a, b, h);
    else if constexpr (kKind == 0 && kK == 3) return p::pmul<f28::kK32>(a, b, h);
    else if constexpr (kKind == 1 && kK == 0) return p::pmul_add<f28::kK4>(a, b, e, h);
    else if constexpr (kKind == 1 && kK == 4) return p::pmul_add<f28::kK32r3>(a, b, e, h);
    else if constexpr (kKind == 2 && kK == 2) return p::psqr<f28::kK16>(a, h);
    else if constexpr (kKind == 2 && kK == 3) return p::psqr<f28::kK32>(a, h);
    else if constexpr (kKind == 3 && kK == 0) return p::psqr_add<f28::kK4>(a, e, h);
    else return p::psqr_add<f28::kK16>(a, e, h);
  }
};

// families 0 and 1 (include/tachyon_mi355x.h lists the ops)
template <class L>
struct FqLimbOps {
  using F = typename L::F;
  using Acc = typename L::Acc;
  using PAcc = typename L::PAcc;
  static constexpr int N = L::N;
  static constexpr int kMaxOp = 64;

  static constexpr LimbShape shape(int op) {
    constexpr int W = L::kWords;
    switch (op) {
      case 0: return {2 * N, N};
      case 1: return {3 * N, N};
      case 2: return {4 * N, N};
      case 3: return {5 * N, N};
      case 4: return {N, N};
      case 5: return {2 * N, N};
      case 6: return {N, N};
      case 7: return {W, N};
      case 8: return {N, W};
      case 9: return {N, 1};
      case 10: return {N, N};
      case 11: return {2 * N, 4 * N + 1};
      case 12: return {6 * N, 4 * N + 1};
      case 13: return {8 * N, 4 * N + 1};
      case 14: return {4 * N, 4 * N + 1};
      case 20: return {2 * N, 2, true};
      case 21: return {4 * N, 8 * N + 2, true};
      case 22: return {12 * N, 8 * N + 2, true};
      case 23: return {16 * N, 8 * N + 2, true};
      case 24: return {8 * N, 8 * N + 2, true};
      default: break;
    }
    if (op >= 32 && op < 64) {
      const int kind = (op - 32) >> 3, k = (op - 32) & 7;
      if (!L::has_pair(kind, k)) return {};
      const int operands = kind == 0 ? 2 : kind == 1 ? 3 : kind == 2 ? 1 : 2;
      return {2 * N * operands, 2 * N, true};
    }
    return {};
  }

  static __device__ __forceinline__ Acc ld_acc(const uint32_t* p) {
    return {ld_limbs<F>(p), ld_limbs<F>(p + N), ld_limbs<F>(p + 2 * N), ld_limbs<F>(p + 3 * N)};
  }
  // lane h's component of Fq2 value number v of an element
  static __device__ __forceinline__ F ld_half(const uint32_t* p, int v, bool h) { return ld_limbs<F>(p + (2 * v + h) * N); }
  static __device__ __forceinline__ PAcc ld_pacc(const uint32_t* p, int v, bool h) {
    return {ld_half(p, v, h), ld_half(p, v + 1, h), ld_half(p, v + 2, h), ld_half(p, v + 3, h)};
  }

  template <int kOp>
  static __device__ __forceinline__ void run(const uint32_t* in, uint32_t* out, bool h) {
    if constexpr (kOp == 0) st_limbs(out, mul(ld_limbs<F>(in), ld_limbs<F>(in + N)));
    else if constexpr (kOp == 1) st_limbs(out, mul_add(ld_limbs<F>(in), ld_limbs<F>(in + N), ld_limbs<F>(in + 2 * N)));
    else if constexpr (kOp == 2)
      st_limbs(out, mul2_add(ld_limbs<F>(in), ld_limbs<F>(in + N), ld_limbs<F>(in + 2 * N), ld_limbs<F>(in + 3 * N)));
    else if constexpr (kOp == 3)
      st_limbs(out, L::mul2_add5(ld_limbs<F>(in), ld_limbs<F>(in + N), ld_limbs<F>(in + 2 * N), ld_limbs<F>(in + 3 * N),
                                 ld_limbs<F>(in + 4 * N)));
    else if constexpr (kOp == 4) st_limbs(out, sqr(ld_limbs<F>(in)));
    else if constexpr (kOp == 5) st_limbs(out, sqr_add(ld_limbs<F>(in), ld_limbs<F>(in + N)));
    else if constexpr (kOp == 6) st_limbs(out, normalize(ld_limbs<F>(in)));
    else if constexpr (kOp == 7) {
      uint32_t w[L::kWords];
#pragma unroll
      for (int i = 0; i < L::kWords; ++i) w[i] = in[i];
      st_limbs(out, L::from32(w));
    } else if constexpr (kOp == 8) {
      uint32_t w[L::kWords];
      to32(ld_limbs<F>(in), w);
#pragma unroll
      for (int i = 0; i < L::kWords; ++i) out[i] = w[i];
    } else if constexpr (kOp == 9) out[0] = is_zero_mod_p(ld_limbs<F>(in)) ? 1u : 0u;
    else if constexpr (kOp == 10) st_limbs(out, L::reduce(ld_limbs<F>(in)));
    else if constexpr (kOp >= 11 && kOp <= 14) {
      int special = 0;
      Acc c;
      if constexpr (kOp == 11) c = L::from_shifted(ld_limbs<F>(in), ld_limbs<F>(in + N));
      else if constexpr (kOp == 12) c = L::madd(ld_acc(in), ld_limbs<F>(in + 4 * N), ld_limbs<F>(in + 5 * N), &special);
      else if constexpr (kOp == 13) c = L::add(ld_acc(in), ld_acc(in + 4 * N), &special);
      else c = L::dbl(ld_acc(in));
      st_limbs(out, c.x);
      st_limbs(out + N, c.y);
      st_limbs(out + 2 * N, c.zz);
      st_limbs(out + 3 * N, c.zzz);
      out[4 * N] = (uint32_t)special;
    } else if constexpr (kOp == 20) out[h] = L::pzero(ld_half(in, 0, h)) ? 1u : 0u;
    else if constexpr (kOp >= 21 && kOp <= 24) {
      int special = 0;
      PAcc c;
      if constexpr (kOp == 21) c = L::pfrom_shifted(ld_half(in, 0, h), ld_half(in, 1, h), h);
      else if constexpr (kOp == 22) c = L::pmadd(ld_pacc(in, 0, h), ld_half(in, 4, h), ld_half(in, 5, h), h, &special);
      else if constexpr (kOp == 23) c = L::padd(ld_pacc(in, 0, h), ld_pacc(in, 4, h), h, &special);
      else c = L::pdbl(ld_pacc(in, 0, h), h);
      st_limbs(out + h * N, c.x);
      st_limbs(out + (2 + h) * N, c.y);
      st_limbs(out + (4 + h) * N, c.zz);
      st_limbs(out + (6 + h) * N, c.zzz);
      out[8 * N + h] = (uint32_t)special;
    } else {
      constexpr int kKind = (kOp - 32) >> 3, kK = (kOp - 32) & 7;
      const F a = ld_half(in, 0, h);
      // operands: pmul a b, pmul_add a b e, psqr a, psqr_add a e
      const F b = kKind <= 1 ? ld_half(in, 1, h) : a;
      const F e = kKind == 1 ? ld_half(in, 2, h) : kKind == 3 ? ld_half(in, 1, h) : a;
      st_limbs(out + h * N, L::template pair_product<kKind, kK>(a, b, e, h));
    }
  }
};

// family 2: BN254 Fr, the NTT butterflies' arithmetic (field/fr29.h)
struct Fr29LimbOps {
  using F = f29::F29;
  static constexpr int N = 9;
  static constexpr int kMaxOp = 10;
  static constexpr LimbShape shape(int op) {
    switch (op) {
      case 0: return {2 * N, N};
      case 1: return {3 * N, N};
      case 2: return {N, N};
      case 3: return {8, N};
      case 4: return {N, 8};
      case 5: return {12 * N, 4 * N};
      case 6: return {8 * N, 4 * N};
      case 7: return {6 * N, 4 * N};
      case 8: return {4 * N, 2 * N};
      case 9: return {2 * N, 2 * N};
      default: return {};
    }
  }
  static __device__ __forceinline__ fr29::TwShoup29 ld_shoup(const uint32_t* p) { return {ld_limbs<F>(p), ld_limbs<F>(p + N)}; }
  template <int kOp>
  static __device__ __forceinline__ void run(const uint32_t* in, uint32_t* out, bool) {
    if constexpr (kOp == 0) st_limbs(out, fr29::mont(ld_limbs<F>(in), ld_limbs<F>(in + N)));
    else if constexpr (kOp == 1) st_limbs(out, fr29::shoup(ld_limbs<F>(in), ld_limbs<F>(in + N), ld_limbs<F>(in + 2 * N)));
    else if constexpr (kOp == 2) st_limbs(out, fr29::reduce(ld_limbs<F>(in)));
    else if constexpr (kOp == 3) {
      uint32_t w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = in[i];
      st_limbs(out, fr29::from_words(w));
    } else if constexpr (kOp == 4) {
      uint32_t w[8];
      fr29::to_canonical_words(ld_limbs<F>(in), w);
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = w[i];
    } else if constexpr (kOp >= 5 && kOp <= 7) {
      F x[4] = {ld_limbs<F>(in), ld_limbs<F>(in + N), ld_limbs<F>(in + 2 * N), ld_limbs<F>(in + 3 * N)};
      const uint32_t* t = in + 4 * N;
      if constexpr (kOp == 5) fr29::radix4(x, ld_shoup(t), ld_shoup(t + 2 * N), ld_shoup(t + 4 * N), ld_shoup(t + 6 * N));
      else if constexpr (kOp == 6)
        fr29::radix4(x, fr29::TwMont29{ld_limbs<F>(t)}, fr29::TwMont29{ld_limbs<F>(t + N)},
                     fr29::TwMont29{ld_limbs<F>(t + 2 * N)}, fr29::TwMont29{ld_limbs<F>(t + 3 * N)});
      else fr29::radix4_last(x, ld_shoup(t));
#pragma unroll
      for (int i = 0; i < 4; ++i) st_limbs(out + i * N, x[i]);
    } else {
      F x[2] = {ld_limbs<F>(in), ld_limbs<F>(in + N)};
      if constexpr (kOp == 8) fr29::radix2(x, ld_shoup(in + 2 * N));
      else fr29::radix2_last(x);
      st_limbs(out, x[0]);
      st_limbs(out + N, x[1]);
    }
  }
};

template <class Ops, int kOp>
__global__ __launch_bounds__(kBlock) void limb_op_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                         size_t count) {
  constexpr LimbShape s = Ops::shape(kOp);
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t e = s.pair ? t >> 1 : t;  // pair-uniform: both lanes of a pair leave together
  if (e >= count) return;
  Ops::template run<kOp>(in + e * s.in, out + e * s.out, s.pair && (t & 1));
}

// op == kOp: the shape (words != nullptr) or the launch; false otherwise
template <class Ops, int kOp>
bool limb_op_one(int op, const uint32_t* in, uint32_t* out, size_t count, int* words) {
  constexpr LimbShape s = Ops::shape(kOp);
  if constexpr (s.in == 0) {
    return false;
  } else {
    if (op != kOp) return false;
    if (words) {
      words[0] = s.in;
      words[1] = s.out;
      return true;
    }
    if (count == 0) return true;
    DeviceBuffer din, dout;
    const size_t ib = count * s.in * sizeof(uint32_t), ob = count * s.out * sizeof(uint32_t);
    TA_HIP(hipMemcpy(din.ensure(ib), in, ib, hipMemcpyHostToDevice));
    uint32_t* d_out = static_cast<uint32_t*>(dout.ensure(ob));
    TA_HIP(hipMemset(d_out, 0, ob));
    const size_t threads = s.pair ? 2 * count : count;
    hipLaunchKernelGGL((limb_op_kernel<Ops, kOp>), dim3(ceil_div(threads, kBlock)), dim3(kBlock), 0, 0,
                       din.as<uint32_t>(), d_out, count);
    TA_HIP(hipGetLastError());
    TA_HIP(hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost));
    return true;
  }
}
template <class Ops, int... kOps>
bool limb_op_any(int op, const uint32_t* in, uint32_t* out, size_t count, int* words,
                 std::integer_sequence<int, kOps...>) {
  return (limb_op_one<Ops, kOps>(op, in, out, count, words) || ...);
}
template <class Ops>
bool limb_op_family(int op, const uint32_t* in, uint32_t* out, size_t count, int* words) {
  return limb_op_any<Ops>(op, in, out, count, words, std::make_integer_sequence<int, Ops::kMaxOp>{});
}
bool limb_op_dispatch(int family, int op, const uint32_t* in, uint32_t* out, size_t count, int* words) {
  switch (family) {
    case 0: return limb_op_family<FqLimbOps<Limb29>>(op, in, out, count, words);
    case 1: return limb_op_family<FqLimbOps<Limb28>>(op, in, out, count, words);
    case 2: return limb_op_family<Fr29LimbOps>(op, in, out, count, words);
    default: return false;
  }
}

}  // namespace

void limb_op(int family, int op, const uint32_t* in, uint32_t* out, size_t count) {
  if (!limb_op_dispatch(family, op, in, out, count, nullptr))
    throw std::runtime_error("tachyon_mi355x_limb_op: unknown family or op");
}

bool limb_op_words(int family, int op, int* in_words, int* out_words) {
  int words[2] = {0, 0};
  const bool ok = limb_op_dispatch(family, op, nullptr, nullptr, 0, words);
  *in_words = words[0];
  *out_words = words[1];
  return ok;
}

void batch_evaluate_bn254_fr(const void* num, const void* den, void* out, size_t n) {
  if (n == 0) return;
  using F = Bn254Fr;
  constexpr uint32_t kChunk = 32;
  DeviceBuffer dn, dd, dout, dpre;
  const size_t bytes = n * sizeof(F);
  TA_HIP(hipMemcpy(dn.ensure(bytes), num, bytes, hipMemcpyHostToDevice));
  TA_HIP(hipMemcpy(dd.ensure(bytes), den, bytes, hipMemcpyHostToDevice));
  const size_t threads = (n + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(batch_evaluate_kernel<F>, dim3(ceil_div(threads, kBlock)), dim3(kBlock), 0, 0, dn.as<F>(),
                     dd.as<F>(), static_cast<F*>(dout.ensure(bytes)), static_cast<F*>(dpre.ensure(bytes)), n, kChunk);
  TA_HIP(hipGetLastError());
  TA_HIP(hipMemcpy(out, dout.as<F>(), bytes, hipMemcpyDeviceToHost));
}

void gen_scalars(int field, uint64_t seed, size_t start, size_t n, void* d_out, hipStream_t stream) {
  if (n == 0) return;
  if (field == 1)
    hipLaunchKernelGGL(gen_scalars_kernel<Bn254Fr>, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, stream, seed, start,
                       n, static_cast<Bn254Fr*>(d_out));
  else if (field == 3)
    hipLaunchKernelGGL(gen_scalars_kernel<Bls381Fr>, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, stream, seed,
                       start, n, static_cast<Bls381Fr*>(d_out));
  else
    throw std::runtime_error("tachyon_mi355x_gen_scalars: unknown scalar field");
  TA_HIP(hipGetLastError());
}

void gen_bases(int curve, uint64_t seed, size_t start, size_t n, size_t chunk, void* d_out, hipStream_t stream) {
  if (n == 0) return;
  if (chunk == 0) throw std::runtime_error("tachyon_mi355x_gen_bases: chunk must be > 0");
  const uint64_t chunk0 = start / chunk;
  const size_t chunks = (start - chunk0 * chunk + n + chunk - 1) / chunk;
  dim3 g(ceil_div(chunks, kBlock)), b(kBlock);
  switch (curve) {
    case 0: hipLaunchKernelGGL(gen_bases_kernel<Bn254G1>, g, b, 0, stream, seed, start, n, chunk, chunk0,
                               static_cast<Affine<Bn254Fq>*>(d_out)); break;
    case 1: hipLaunchKernelGGL(gen_bases_kernel<Bn254G2>, g, b, 0, stream, seed, start, n, chunk, chunk0,
                               static_cast<Affine<Bn254Fq2>*>(d_out)); break;
    case 2: hipLaunchKernelGGL(gen_bases_kernel<Bls381G1>, g, b, 0, stream, seed, start, n, chunk, chunk0,
                               static_cast<Affine<Bls381Fq>*>(d_out)); break;
    case 3: hipLaunchKernelGGL(gen_bases_kernel<Bls381G2>, g, b, 0, stream, seed, start, n, chunk, chunk0,
                               static_cast<Affine<Bls381Fq2>*>(d_out)); break;
    default: throw std::runtime_error("tachyon_mi355x_gen_bases: unknown curve");
  }
  TA_HIP(hipGetLastError());
}

void field_op(int field, int op, const void* a, const void* b, void* out, size_t count) {
  switch (field) {
    case 0: run_field_op<Bn254Fq>(op, a, b, out, count); break;
    case 1: run_field_op<Bn254Fr>(op, a, b, out, count); break;
    case 2: run_field_op<Bls381Fq>(op, a, b, out, count); break;
    case 3: run_field_op<Bls381Fr>(op, a, b, out, count); break;
    default: throw std::runtime_error("tachyon_mi355x_field_op: unknown field");
  }
}

void ec_op(int curve, int op, const void* a, const void* b, void* out, size_t count) {
  switch (curve) {
    case 0: run_ec_op<Bn254Fq>(op, a, b, out, count); break;
    case 1: run_ec_op<Bn254Fq2>(op, a, b, out, count); break;
    case 2: run_ec_op<Bls381Fq>(op, a, b, out, count); break;
    case 3: run_ec_op<Bls381Fq2>(op, a, b, out, count); break;
    default: throw std::runtime_error("tachyon_mi355x_ec_op: unknown curve");
  }
}

}  // namespace tachyon_amd::util
